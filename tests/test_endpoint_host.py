"""Stream endpointing (SPEC.md 1.17, include/lsm_hip_endpoint.h), what can be checked without a GPU: the NumPy restatement
(tests/endpoint_restatement.py) against hand-built cases with known answers, its cut invariance, the closure bound, the
launch function's refusals (made before any device work, so they run here), the state machine and the addressing as a host
program under AddressSanitizer, the build lists, classify.py's flags, and the coverage of the seeded streams the GPU tests
(test_gpu_endpoint.py) push: a run that exercises nothing cannot pass there."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endpoint_restatement as ER  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_endpoint_state_bytes", "lsm_endpoint_max_utterances", "lsm_endpoint_stream_f32")
HOP = 160
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------
def _levels(levels):
    """One stream whose bin j is 160 samples of ``levels[j]``: e_j = 160 * level^2, exact for powers of two."""
    return np.repeat(np.asarray(levels, dtype=np.float32), HOP)[None, :]


def _run(levels, finish=False, **kw):
    """The restatement on one stream in one push, activity = "the level is not zero" unless ``kw`` says otherwise: ``(list of
    (first, bins, flags), out, state)``."""
    p = ER.params(**{**dict(ratio=0.0, floor=0.0, W=1), **kw})
    st = [ER.fresh()]
    audio = _levels(levels)
    out = ER.push(st, audio, None, [1] if finish else None, p, ER.max_utterances_padded(len(levels), p["P"], p["G"], p["M"]))
    return [(f, b, fl) for _, f, b, fl, _ in ER.listing(out)], out, st[0]


def test_a_word_closes_at_last_plus_pad_and_the_preroll_stops_at_the_start_and_at_avail():
    got, out, st = _run([0, 0, 1, 1, 1, 0, 0, 0, 0, 0], P=1, G=2, A=3, M=20)
    assert got == [(1, 5, 0)] and out["count"].tolist() == [1] and st["mode"] == 0 and st["avail"] == 6
    # the emitted samples are the stream's [160 s, 160 (end + 1)), the rest of the row +0.0
    assert out["audio"][0, 0, :5 * HOP].tobytes() == _levels([0, 1, 1, 1, 0]).tobytes() and not out["audio"][0, 0, 5 * HOP:].any()
    assert _run([0, 1, 1, 1, 0, 0, 0, 0, 0, 0], P=3, G=3, A=3, M=20)[0] == [(0, 7, 0)]          # s = max(1 - 3, 0)
    got, _, st = _run([1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0], P=2, G=3, A=3, M=20)
    assert got == [(0, 5, 0), (5, 6, 0)] and "preroll_avail" in st["events"]                   # s = max(6 - 2, avail = 5)


def test_a_click_is_dropped_and_a_long_word_is_cut():
    got, out, st = _run([0, 0, 1, 0, 0, 0, 0], P=0, G=2, A=3, M=20)
    assert got == [] and out["count"].tolist() == [0] and st["events"] == ["click"] and st["avail"] == 3
    assert _run([0, 1, 1, 0, 0, 0, 0], P=0, G=2, A=3, M=20)[0] == []                            # two active bins: still a click
    assert _run([0, 1, 0, 1, 0, 0, 0], P=0, G=2, A=3, M=20)[0] == [(1, 3, 0)]                   # last - f + 1 = 3: kept
    got, _, st = _run([1] * 9 + [0, 0], P=0, G=2, A=3, M=6)
    assert got == [(0, 6, ER.CUT), (6, 3, 0)] and st["events"] == ["cut", "normal"]
    # a cut word is kept whatever its active span: M = 4 bins of which one is active, through the pre-roll
    assert _run([0, 0, 0, 0, 1], P=3, G=3, A=3, M=4)[0] == [(1, 4, ER.CUT)]


def test_the_hang_wins_over_the_length_on_the_same_bin():
    assert _run([1, 1, 1, 0, 0], P=0, G=2, A=3, M=5)[0] == [(0, 3, 0)]                          # bin 4: n - last = 2, n - s + 1 = 5
    assert _run([1, 1, 1, 1, 0], P=0, G=2, A=3, M=5)[0] == [(0, 5, ER.CUT)]                     # bin 4: n - last = 1


def test_ties_are_inactive():
    # E * ratio: e_0 = 160, e_1 = 160 / 4 = E * 0.25 exactly
    _, out, _ = _run([1, 0.5, 0.5], ratio=0.25, W=2, P=0, G=1, A=3, M=3)
    assert out["energy"][0].tolist() == [160.0, 40.0, 40.0] and out["active"][0].tolist() == [1, 0, 1]
    above = np.nextafter(np.float32(0.5), np.float32(1))
    assert _run([1, above, 0], ratio=0.25, W=2, P=0, G=1, A=3, M=3)[1]["active"][0].tolist() == [1, 1, 0]
    # the floor: e = 40 against a floor of 40, and of the float64 below it
    assert _run([0.5, 1, 0.5], floor=40.0, P=0, G=1, A=3, M=3)[1]["active"][0].tolist() == [0, 1, 0]
    assert _run([0.5, 1, 0.5], floor=np.nextafter(40.0, 0.0), P=0, G=1, A=3, M=3)[1]["active"][0].tolist() == [1, 1, 1]
    # ratio = 0 and an all-zero bin: 0 > 0 is false
    assert _run([0, 0, 0])[1]["active"][0].tolist() == [0, 0, 0]


def test_a_nan_bin_is_inactive_and_its_samples_arrive_as_words():
    audio = _levels([1, 1, 1, 1, 1, 0, 0, 0])
    audio[0, 2 * HOP + 7] = np.float32(np.nan)
    audio.view(np.uint32)[0, 2 * HOP + 8] = 0x7FC12345                                          # a NaN with a payload
    audio[0, 3 * HOP + 1] = np.float32(np.inf)                                                  # e = +inf
    audio[0, 4 * HOP + 5] = np.float32(3e38)                                                    # 9e76: finite in float64, loud
    audio[0, 4 * HOP + 2] = np.float32(-0.0)
    p = ER.params(ratio=0.0, floor=0.0, W=3, P=0, G=3, A=3, M=8)
    out = ER.push([ER.fresh()], audio, None, None, p, 5)
    assert np.isnan(out["energy"][0, 2]) and np.isinf(out["energy"][0, 3]) and 8e76 < out["energy"][0, 4] < 1e77
    assert out["active"][0].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]                                # and the next window is not poisoned
    assert ER.listing(out) == [(0, 0, 5, 0, audio[0, :5 * HOP].tobytes())]
    row = out["audio"][0, 0].view(np.uint32)
    assert row[2 * HOP + 8] == 0x7FC12345 and row[4 * HOP + 2] == 0x80000000 and not row[5 * HOP:].any()


def test_a_loud_word_silences_a_quiet_one_for_the_window_and_no_longer():
    W = 4
    _, out, _ = _run([1] + [0.25] * 6, ratio=0.1, W=W, P=0, G=8, A=3, M=20)                     # 10 > 160 * 0.1 is false
    assert out["active"][0].tolist() == [1, 0, 0, 0, 1, 1, 1]                                   # bins 1 .. W - 1 see bin 0; bin W does not
    assert _run([1] + [0.25] * 6, ratio=0.1, W=W + 1, P=0, G=8, A=3, M=20)[1]["active"][0].tolist() == [1, 0, 0, 0, 0, 1, 1]


def test_finish_while_open_and_while_idle():
    got, _, st = _run([0, 1, 1, 1], finish=True, P=2, G=4, A=3, M=20)
    assert got == [(0, 4, ER.FLUSHED)] and st["n"] == 0 and st["mode"] == 0 and st["avail"] == 0 and len(st["tail"]) == 0
    assert _run([0, 1, 1, 1, 0, 0, 0], finish=True, P=2, G=4, A=3, M=20)[0] == [(0, 6, ER.FLUSHED)]      # end = last + P < last bin
    assert _run([0, 1], finish=True, P=0, G=4, A=3, M=20)[0] == []                                       # a flushed click
    got, _, st = _run([0, 0, 0, 0], finish=True, P=2, G=4, A=3, M=20)
    assert got == [] and st["n"] == 0
    # a finish with no hops flushes what earlier pushes left open, from the history
    p = ER.params(ratio=0.0, floor=0.0, W=1, P=1, G=4, A=3, M=20)
    st = [ER.fresh()]
    assert ER.listing(ER.push(st, _levels([0, 1, 1, 1]), None, None, p, 3)) == []
    out = ER.push(st, _levels([9, 9, 9, 9]), [0], [1], p, 3)
    assert ER.listing(out) == [(0, 0, 4, ER.FLUSHED, _levels([0, 1, 1, 1]).tobytes())]


# ---- seeded streams: the GPU tests' cases and the cut invariance ----------------------------------------------------------------
N_STREAMS, N_PUSHES = 5, 6
GPU_HOPS = (1, 7, 64, 65)
# (W, P, G, M): W in {1, 8}, P in {0, 3}, G in {1, 4}, M in {3, 12}, every combination the ranges allow (P < M, P <= G)
GPU_COMBOS = tuple((W, P, G, M) for W in (1, 8) for P, G in ((0, 1), (0, 4), (3, 4)) for M in (3, 12) if P < M)
RATIO, FLOOR = 1e-2, 1e-3


def timeline(n_bins, G, M, rng, special=None):
    """A stream of ``n_bins`` bins: runs of noise at 0.3 (speech: 1 to M + 4 bins, clicks included) between runs of noise at
    0.0005 (1 to G + 3 bins), under the floor.  ``special``: "nan" / "huge" put one such sample into a speech bin, "negzero"
    makes some quiet bins -0.0 words."""
    x = np.zeros(n_bins * HOP, dtype=np.float32)
    at, on = 0, bool(rng.integers(0, 2))
    while at < n_bins:
        run = int(rng.integers(1, M + 5)) if on else int(rng.integers(1, G + 4))
        hi = min(n_bins, at + run)
        x[at * HOP:hi * HOP] = (rng.standard_normal((hi - at) * HOP) * (0.3 if on else 0.0005)).astype(np.float32)
        if not on and special == "negzero" and rng.integers(0, 2):
            x[at * HOP:hi * HOP] = np.float32(-0.0)
        if on and special in ("nan", "huge") and hi - at >= 2:
            x[(at + 1) * HOP + 11] = np.float32(np.nan) if special == "nan" else np.float32(3e38)
        at, on = hi, not on
    return x


@functools.lru_cache(maxsize=None)
def gpu_case(n_hops, combo):
    """The pushes of one GPU case, from a fixed seed: ``dict(p, max_utts, audio [6 x (5, n_hops * 160)], hops [6 x 5 raw int32
    values, None for push 4], finish [6 x 5, None for push 1])``.  The raw hop values include -1, 0, n_hops + 5, INT32_MIN and INT32_MAX; what
    lies behind a stream's clamped hops in its row is NaN, which must not be read."""
    W, P, G, M = GPU_COMBOS[combo]
    rng = np.random.default_rng(1000 * n_hops + combo)
    specials = [None, "nan", "huge", "negzero", None]
    lines = [timeline(N_PUSHES * n_hops, G, M, rng, specials[b]) for b in range(N_STREAMS)]
    seen = [0] * N_STREAMS
    audio, hops, finish = [], [], []
    for k in range(N_PUSHES):
        raw = []
        for b in range(N_STREAMS):
            choice = int(rng.integers(0, 8))
            raw.append([n_hops, n_hops, n_hops, int(rng.integers(0, n_hops + 1)), 0, -1, n_hops + 5, I32_MAX][choice]
                       if b else [n_hops, I32_MIN, n_hops + 5, 0, I32_MAX, n_hops][k])
        if k == 4:                                                  # a NULL stream_hops: every stream runs n_hops
            raw = [n_hops] * N_STREAMS
        block = np.full((N_STREAMS, n_hops * HOP), np.nan, dtype=np.float32)
        for b in range(N_STREAMS):
            h = ER.clamp_hops(raw[b], n_hops)
            block[b, :h * HOP] = lines[b][seen[b] * HOP:(seen[b] + h) * HOP]
            seen[b] += h
        audio.append(block)
        hops.append(None if k == 4 else raw)
        # stream 1 ends in the middle of the run, stream 0 with no hops (push 3: its raw count is 0), everything at the end;
        # push 1 passes a NULL finish
        finish.append(None if k == 1 else [1 if (k == N_PUSHES - 1 or (b == 1 and k == 2) or (b == 0 and k == 3)) else 0
                                           for b in range(N_STREAMS)])
    return dict(p=ER.params(RATIO, FLOOR, W, P, G, 3, M), max_utts=ER.max_utterances_padded(n_hops, P, G, M), audio=audio,
                hops=hops, finish=finish)


def prefill(case, k):
    """What the output buffers of push ``k`` hold before it: bytes of 0xAA, so that "left alone" and "written" can be told."""
    n_hops, M, U = case["audio"][k].shape[1] // HOP, case["p"]["M"], case["max_utts"]
    fill = lambda shape, dtype: np.frombuffer(b"\xaa" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape)  # noqa: E731
    return dict(audio=fill((N_STREAMS, U, HOP * M), np.float32), bins=fill((N_STREAMS, U), np.int32),
                first=fill((N_STREAMS, U), np.int64), flags=fill((N_STREAMS, U), np.int32), count=fill((N_STREAMS,), np.int32),
                energy=fill((N_STREAMS, n_hops), np.float64), active=fill((N_STREAMS, n_hops), np.uint8))


@functools.lru_cache(maxsize=None)
def gpu_expected(n_hops, combo):
    """The restatement's arrays of every push of a case (computed once, shared, not to be changed) and the events of its run."""
    case = gpu_case(n_hops, combo)
    states = [ER.fresh() for _ in range(N_STREAMS)]
    with np.errstate(all="ignore"):
        outs = [ER.push(states, case["audio"][k], case["hops"][k], case["finish"][k], case["p"], case["max_utts"],
                        prefill(case, k)) for k in range(N_PUSHES)]
    return outs, [e for st in states for e in st["events"]]


def test_the_gpu_streams_exercise_every_path():
    """The coverage condition, on the restatement alone."""
    events, emitted = [], 0
    for n_hops in GPU_HOPS:
        for combo in range(len(GPU_COMBOS)):
            outs, ev = gpu_expected(n_hops, combo)
            events += ev
            emitted += sum(int(o["count"].sum()) for o in outs)
            for o in outs:                                          # no case loses an utterance to full slots
                assert (o["count"] < gpu_case(n_hops, combo)["max_utts"]).all() or n_hops == 1
    for what in ("normal", "cut", "click", "preroll_avail", "spans_push", "flushed", "no_hops"):
        assert events.count(what) >= 3, (what, events.count(what))
    assert emitted >= 200
    # per push length: something is emitted, and an utterance spans a push boundary
    for n_hops in GPU_HOPS:
        ev = [e for combo in range(len(GPU_COMBOS)) for e in gpu_expected(n_hops, combo)[1]]
        assert "spans_push" in ev and ("normal" in ev or "cut" in ev), n_hops
    # NaN and 3e38 samples and -0.0 words arrive inside emitted utterances
    words = np.concatenate([o["audio"][b, u, :HOP * int(o["bins"][b, u])].view(np.uint32)
                            for outs in (gpu_expected(64, c)[0] for c in range(len(GPU_COMBOS))) for o in outs
                            for b in range(N_STREAMS) for u in range(int(o["count"][b]))])
    values = words.view(np.float32)
    assert np.isnan(values).any() and (values == np.float32(3e38)).any() and (words == 0x80000000).any()


def _delivered(case):
    """Per stream the samples a case delivers, push after push (a finish in between makes the later ones a new stream)."""
    n_hops = case["audio"][0].shape[1] // HOP
    return [np.concatenate([case["audio"][k][b, :ER.clamp_hops(None if case["hops"][k] is None else case["hops"][k][b], n_hops) * HOP]
                            for k in range(N_PUSHES)]) for b in range(N_STREAMS)]


def _all_utterances(lines, p, cuts_of, rng):
    """Every stream of ``lines`` pushed in the pieces ``cuts_of(n_bins, rng)`` names, a finish with the last piece: the
    utterance lists, concatenated over the pushes."""
    found = []
    for x in lines:
        n_bins = len(x) // HOP
        st = [ER.fresh()]
        mine, at = [], 0
        pieces = cuts_of(n_bins, rng)
        assert sum(pieces) == n_bins
        for i, h in enumerate(pieces):
            H = max(h, 1)
            row = np.full((1, H * HOP), np.nan, dtype=np.float32)
            row[0, :h * HOP] = x[at * HOP:(at + h) * HOP]
            out = ER.push(st, row, [h], [1 if i == len(pieces) - 1 else 0], p, ER.max_utterances_padded(H, p["P"], p["G"], p["M"]))
            mine += [(f, b, fl, raw) for _, f, b, fl, raw in ER.listing(out)]
            at += h
        found.append(mine)
    return found


def _random_cuts(n_bins, rng):
    pieces = []
    while sum(pieces) < n_bins:
        pieces.append(min(int(rng.integers(0, 12)) * int(rng.integers(0, 2)), n_bins - sum(pieces)))
    return pieces + [0]


def test_the_restatement_is_cut_invariant():
    """One piece, hop by hop and random splits with empty pushes: the same utterances, byte for byte."""
    rng = np.random.default_rng(5)
    total = 0
    with np.errstate(all="ignore"):
        for W, P, G, M in ((8, 3, 4, 12), (1, 0, 1, 3), (100, 3, 20, 100)):
            lines = [timeline(90, G, M, rng, sp) for sp in (None, "nan", "negzero")]
            p = ER.params(RATIO, FLOOR, W, P, G, 3, M)
            whole = _all_utterances(lines, p, lambda n, r: [n], rng)
            assert whole == _all_utterances(lines, p, lambda n, r: [1] * n, rng)
            assert whole == _all_utterances(lines, p, _random_cuts, rng)
            total += sum(len(w) for w in whole)
            for per in whole:                                       # utterances never overlap; a kept one has 3 .. M bins
                assert all(3 <= b <= M for _, b, _, _ in per)
                assert all(f0 + b0 <= f1 for (f0, b0, _, _), (f1, _, _, _) in zip(per, per[1:]))
    assert total >= 12


# ---- the closure bound ----------------------------------------------------------------------------------------------------------
def _kept(levels, P, G, M, before=()):
    """Kept utterances of the LAST ``len(levels)`` bins, behind the bins ``before`` of an earlier push that closes nothing."""
    p = ER.params(ratio=0.0, floor=0.0, W=1, P=P, G=G, A=3, M=M)
    st = [ER.fresh()]
    if len(before):
        assert not ER.push(st, _levels(before), None, None, p, 10 ** 4)["count"].any()
    return int(ER.push(st, _levels(levels), None, None, p, 10 ** 4)["count"][0])


def test_the_closure_bound():
    """`lsm_endpoint_max_utterances` minus the finish slot.  Nothing exceeds it on the grid, for pad_bins = 0 and pad_bins =
    hang_bins (clamped below max_bins).  The bound's divisor is min(G + 1, M): "an active bin plus G quiet ones, or M bins".
    A KEPT utterance that closes by silence needs 3 active bins first (min_span_bins >= 3), G + 3 bins in all, so the pace an
    envelope can reach is min(G + 3, M): forced cuts where M <= G + 3 (M - 1 open bins before the push, then activity
    throughout: a cut at bin 0 and every M bins), closes by silence otherwise (three active bins and G - 1 quiet ones before the
    push, then a quiet bin, three active bins, G quiet ones, ...).  The adversarial envelope reaches 1 + (H - 1) / pace, which
    IS the bound minus the finish slot wherever (H - 1) / pace = (H - 1) / min(G + 1, M) -- every M <= G + 1 and the short
    pushes of the others."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(11)
    reached = 0
    for H in (1, 2, 7, 30, 64):
        for G, M in ((1, 3), (4, 3), (4, 5), (11, 12), (2, 12), (4, 12)):
            bound = lib.lsm_endpoint_max_utterances(H, G, M)
            assert bound == ER.max_utterances(H, G, M) == 2 + (H - 1) // min(G + 1, M)
            pace = min(G + 3, M)
            if M <= G + 3:
                before, adversarial = [1] * (M - 1), [1] * H
            else:
                before, adversarial = [1, 1, 1] + [0] * (G - 1), ([0] + ([1, 1, 1] + [0] * G) * H)[:H]
            got = _kept(adversarial, 0, G, M, before)
            assert got == 1 + (H - 1) // pace <= bound - 1, (H, G, M, got)
            reached += got == bound - 1
            assert (got == bound - 1) == ((H - 1) // pace == (H - 1) // min(G + 1, M)), (H, G, M)
            for P in {0, min(G, M - 1)}:
                for _ in range(6):
                    levels = (rng.random(H) < rng.uniform(0.2, 0.95)).astype(np.float32)
                    for n_open in (0, min(M - 1, 3)):
                        assert _kept(levels, P, G, M, [1] * n_open) <= bound - 1, (H, P, G, M)
    assert reached >= 18


def test_a_pad_between_the_two_regimes_needs_the_padded_bound():
    """max_bins >= hang_bins + 3 and max_bins - hang_bins - 1 < pad_bins < 2 hang_bins + 1 - max_bins: a forced cut follows a
    close by silence after max(M - P, M + P - G) bins, fewer than min(G + 1, M).  G = 10, M = 13, P = 5: 8 against 11.  The
    library's figure is passed at H = 4000; `frontend.endpoint_max_utterances` (what `EndpointStream` allocates) is not."""
    from lsm_speech_classifier_amd import frontend
    P, G, M, H = 5, 10, 13, 4000
    assert ER.closure_spacing(P, G, M) == 8 and ER.closure_spacing(0, G, M) == ER.closure_spacing(G, G, M) == 11
    assert ER.closure_spacing(3, 20, 100) == 21 and ER.closure_spacing(3, 4, 12) == 5 and ER.closure_spacing(0, 1, 3) == 2
    env = np.zeros(H, dtype=np.float32)
    env[0:3] = 1
    c = 2 + G
    while c + 30 < H:
        cut = c - G + P + M                                         # avail = c - G + P + 1: the cut comes M - 1 bins behind it
        env[c + 1:cut + 4] = 1                                      # ... and three active bins start the next word
        c = cut + 3 + G
    got = _kept(env, P, G, M)
    assert ER.max_utterances(H, G, M) - 1 < got <= ER.max_utterances_padded(H, P, G, M) - 1
    for h, p, g, m in ((H, P, G, M), (100, 3, 20, 100), (65, 3, 4, 12), (1, 0, 1, 3), (4096, 0, 1, 3)):
        assert frontend.endpoint_max_utterances(h, p, g, m) == ER.max_utterances_padded(h, p, g, m) >= ER.max_utterances(h, g, m)
    # slots that are full drop the utterance and nothing else: the count saturates, the later state is the same
    p = ER.params(ratio=0.0, floor=0.0, W=1, P=P, G=G, A=3, M=M)
    few, many = [ER.fresh()], [ER.fresh()]
    a = ER.push(few, _levels(env), None, None, p, 5)
    b = ER.push(many, _levels(env), None, None, p, 600)
    assert a["count"].tolist() == [5] and ER.listing(a) == ER.listing(b)[:5]
    assert {k: v for k, v in few[0].items() if k not in ("events", "tail")} == {k: v for k, v in many[0].items()
                                                                                if k not in ("events", "tail")}


# ---- header, binding, build -----------------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_the_three_names():
    import re
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_endpoint.h")).read()
    assert _lib.ENDPOINT_SYMBOLS == tuple(_lib.ENDPOINT_SIGS) == NEW
    for name in NEW:
        m = re.search(r"^(?:int|long) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, f"{name} is not declared"
        params = [" ".join(q.split()) for q in m.group(1).split(",")]
        res, args = _lib.ENDPOINT_SIGS[name]
        assert len(args) == len(params) and res is (C.c_long if name.endswith("state_bytes") else _lib.c_int)
        for q, ctype in zip(params, args):
            want = _lib.c_void if "*" in q else _lib.c_double if q.startswith("double ") else _lib.c_int
            assert ctype is want, f"{name}: {q}"
        assert name not in _lib._SIGS
    lib = _lib.load()
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert "lsm_hip_endpoint.h" in build.ABI_HEADERS and "endpoint.hip" in build.SOURCES
    assert {"endpoint_body.h", "bin_energy.h", "trim_body.h"} <= set(build.HEADERS)
    assert len(build.PUBLIC_HEADERS) == 9 and "lsm_hip_endpoint.h" not in build.PUBLIC_HEADERS
    with pytest.raises(OSError):                                    # the header is hashed into the build id
        build.source_id(include_dir=os.path.join(ROOT, "lsm-speech-classifier_amd"))
    # the energy code is one copy: both kernels include it, neither spells the sum out
    for src in ("trim.hip", "endpoint.hip"):
        text = open(os.path.join(ROOT, "lsm-speech-classifier_amd", "csrc", src)).read()
        assert '#include "bin_energy.h"' in text and "lsm_energy::row_energy" in text and "acc += x * x" not in text


def test_state_bytes():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    for W in (1, 2, 3, 8, 100, 1023, 1024):
        for M in (3, 4, 12, 100, 4096):
            n = lib.lsm_endpoint_state_bytes(W, M)
            assert n % 16 == 0 and n >= 8 * (W - 1) + 4 * HOP * M + 5 * 8 + 4, (W, M, n)
    assert lib.lsm_endpoint_state_bytes(1, 3) == 64 + 4 * HOP * 3
    for W, M in ((0, 3), (1025, 3), (1, 2), (1, 4097)):
        assert lib.lsm_endpoint_state_bytes(W, M) < 0
    for H, G, M in ((0, 1, 3), (4097, 1, 3), (1, 0, 3), (1, 1025, 3), (1, 1, 2), (1, 1, 4097)):
        assert lib.lsm_endpoint_max_utterances(H, G, M) < 0


def test_the_refusals_in_their_order():
    """Every refusal is made on the host before anything is launched, so fake (aligned, distinct) addresses serve."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    A, S, T, U, B_, F, L, N, E, V, H_, Q = (0x10000 * (i + 1) for i in range(12))
    good = dict(audio=A, n_streams=2, n_hops=10, hops=H_, finish=Q, ratio=1e-3, floor=0.0, W=8, P=1, G=2, A=3, M=12, state_in=S,
                state_out=T, max_utts=5, utt_audio=U, utt_bins=B_, first=F, flags=L, count=N, energy=E, active=V)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_endpoint_stream_f32(a["audio"] or None, a["n_streams"], a["n_hops"], a["hops"] or None, a["finish"] or None,
                                         C.c_double(a["ratio"]), C.c_double(a["floor"]), a["W"], a["P"], a["G"], a["A"], a["M"],
                                         a["state_in"] or None, a["state_out"] or None, a["max_utts"], a["utt_audio"] or None,
                                         a["utt_bins"] or None, a["first"] or None, a["flags"] or None, a["count"] or None,
                                         a["energy"] or None, a["active"] or None, None)
        return rc, lib.lsm_last_error().decode()

    # each row breaks its own rule AND every later one: the message names the earliest
    later = [dict(n_streams=-1), dict(n_hops=0), dict(ratio=float("nan")), dict(floor=-1.0), dict(W=0), dict(M=2), dict(P=-1),
             dict(G=0), dict(A=2), dict(max_utts=4), dict(utt_bins=0), dict(utt_audio=A), dict(state_out=T + 8)]
    texts = ["n_streams=-1", "n_hops=0", "ratio=", "floor=-1", "window_bins=0", "max_bins=2", "pad_bins=-1", "hang_bins=0",
             "min_span_bins=2", "max_utts=4", "are required", "must not be audio", "16-byte aligned"]
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)
    for kw, text, code in ((dict(n_hops=4097, max_utts=5000), "4096", -4), (dict(ratio=1.0), "ratio=1", -1),
                           (dict(ratio=-0.5), "ratio=-0.5", -1), (dict(ratio=float("inf")), "ratio=inf", -1),
                           (dict(floor=float("inf")), "floor=inf", -1), (dict(floor=float("nan")), "floor=", -1),
                           (dict(W=1025), "window_bins=1025", -1), (dict(M=4097), "max_bins=4097", -1),
                           (dict(P=12), "pad_bins=12", -1), (dict(P=3, G=2), "hang_bins=2", -1), (dict(G=1025), "hang_bins=1025", -1),
                           (dict(A=13), "min_span_bins=13", -1), (dict(audio=0), "are required", -1),
                           (dict(utt_audio=0), "are required", -1), (dict(audio=A + 2), "4-byte aligned", -1),
                           (dict(utt_audio=U + 1), "4-byte aligned", -1), (dict(hops=H_ + 2), "4-byte aligned", -1),
                           (dict(finish=Q + 1), "4-byte aligned", -1), (dict(utt_bins=B_ + 2), "4-byte aligned", -1),
                           (dict(flags=L + 2), "4-byte aligned", -1), (dict(count=N + 3), "4-byte aligned", -1),
                           (dict(first=F + 4), "8-byte aligned", -1), (dict(energy=E + 4), "8-byte aligned", -1),
                           (dict(state_in=S + 8), "16-byte aligned", -1)):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    # max_utts: exactly the library's figure passes the check (the next refusal, or none, answers)
    assert lib.lsm_endpoint_max_utterances(10, 2, 12) == 5 and call(n_streams=0)[0] == 0 and call(n_streams=0, max_utts=4)[0] == -1
    assert call(n_streams=0, hops=0, finish=0, state_in=0, state_out=0, first=0, flags=0, count=0, energy=0, active=0)[0] == 0


def test_the_state_machine_and_the_addressing_under_address_sanitizer(tmp_path):
    """csrc/endpoint_body.h -- the code the kernel runs its machine and forms every address with -- as a host program over hand
    cases, splits and headers that hold anything, built with -fsanitize=address,undefined (tests/endpoint_body_check.cc)."""
    src = os.path.join(ROOT, "tests", "endpoint_body_check.cc")
    exe = str(tmp_path / "endpoint_body_check")
    built = False
    # the runtimes are linked statically: the program then needs nothing of the environment it is started from
    for cxx, static in ((shutil.which("g++"), ["-static-libasan", "-static-libubsan"]), (shutil.which("clang++"), [])):
        if not cxx:
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
                           + ["-I", os.path.join(ROOT, "lsm-speech-classifier_amd", "csrc"), src, "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            built = True
            break
    if not built:
        pytest.skip("no host compiler with the sanitizer runtimes")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "endpoint_body ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the Python layer's host checks and classify.py's flags -------------------------------------------------------------------
def test_endpoint_floor_and_slots():
    from lsm_speech_classifier_amd import frontend
    assert frontend.endpoint_floor(None) == 0.0 and frontend.endpoint_floor(-60.0) == 160 * 10.0 ** -6.0 == ER.floor_of(-60.0)
    assert frontend.endpoint_floor(0) == 160.0 and frontend.trim_ratio(30.0) == ER.ratio_of(30.0)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="floor_db"):
            frontend.endpoint_floor(bad)
    assert frontend.endpoint_max_utterances(100, 3, 20, 100) == 6 and frontend.RAGGED_HOP == HOP
    assert tuple(frontend.Utterances._fields) == ("audio", "bins", "first", "flags", "count")


def test_classify_flags():
    import classify
    ap = classify.build_parser()
    a = ap.parse_args(["--model", "m.npz", "a.wav", "b.wav"])
    old = dict(model="m.npz", files=["a.wav", "b.wav"], stream=False, window_ms=1000.0, hop_ms=100.0, hold=3, background=-1)
    assert {k: v for k, v in vars(a).items() if not k.startswith("endpoint")} == old and a.endpoint is False
    a = ap.parse_args(["--model", "m.npz", "--stream", "--window-ms", "500", "--hop-ms", "50", "a.wav"])
    assert {k: v for k, v in vars(a).items() if not k.startswith("endpoint")} == dict(old, files=["a.wav"], stream=True,
                                                                                       window_ms=500.0, hop_ms=50.0)
    a = ap.parse_args(["--model", "m.npz", "--stream", "--endpoint", "a.wav"])
    assert classify.endpoint_from_args(a, 100) == dict(top_db=30.0, floor_db=-60.0, pad_bins=3, hang_bins=20, min_span_bins=3,
                                                       max_bins=100)
    a = ap.parse_args(["--model", "m.npz", "--stream", "--endpoint", "--endpoint-top-db", "25", "--endpoint-floor-db", "-50",
                       "--endpoint-pad-ms", "50", "--endpoint-hang-ms", "300", "--endpoint-min-ms", "60", "a.wav"])
    assert classify.endpoint_from_args(a, 40) == dict(top_db=25.0, floor_db=-50.0, pad_bins=5, hang_bins=30, min_span_bins=6,
                                                      max_bins=40)
    for bad, text in ((["--endpoint-top-db", "0"], "--endpoint-top-db"), (["--endpoint-pad-ms", "400"], "--endpoint-pad-ms"),
                      (["--endpoint-hang-ms", "20"], "--endpoint-hang-ms"), (["--endpoint-min-ms", "10"], "--endpoint-min-ms"),
                      (["--endpoint-min-ms", "500"], "--endpoint-min-ms")):
        with pytest.raises(SystemExit, match=text):
            classify.endpoint_from_args(ap.parse_args(["--model", "m.npz", "--stream", "--endpoint", "a.wav"] + bad), 40)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "classify.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--endpoint", "--endpoint-top-db", "--endpoint-floor-db",
                                                              "--endpoint-pad-ms", "--endpoint-hang-ms", "--endpoint-min-ms"))
