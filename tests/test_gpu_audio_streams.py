"""Streamed gammatone front end (SPEC.md 1.6, include/lsm_hip_audio.h: `lsm_gammatone_stream_f64`,
`frontend.GammatoneStream`, `frontend.stream_column_plan`, `SpikeFrontEnd.db_range`, `pipeline.AudioStreamBank`).

The references are the plain-C oracle's pieces: `gammatone_spec` for the columns (bit for bit), NumPy's `log10` for the dB
values (1e-12, as everywhere in SPEC.md), and -- from the DEVICE's dB array, so that no libm stands between the two sides
-- NumPy's normalisation and the oracle's `encode_hysteresis` for the raster (bit for bit).  A cut run is compared with the
uncut one byte for byte, state block included.  The code under test is never its own reference."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOP, HOPS, N_STREAMS = 160, 40, 3
THR, GAP = [0.70, 0.80, 0.90, 0.95], 0.1
FILL = 0xAA
FILTERS = (2, 64, 65, 128)                                   # 65: a second, mostly empty wave
ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _ncols(nwin, hops=HOPS):
    return (hops * HOP - nwin) // HOP + 1


def _audio():
    """3 streams of 40 hops of seeded noise under a level ramp of 50 dB up and down again (its peak at another place in
    every stream); stream 2 starts with four hops of exact silence, whose columns lie below the 80 dB floor."""
    if "audio" not in _CACHE:
        rng = np.random.RandomState(20260)
        n = HOPS * HOP
        t = np.arange(n) / n
        audio = np.empty((N_STREAMS, n), dtype=np.float32)
        for b, peak in enumerate((0.5, 0.35, 0.65)):
            level_db = -50.0 * np.abs(t - peak) / max(peak, 1 - peak)
            audio[b] = (rng.standard_normal(n) * 0.3 * 10.0 ** (level_db / 20.0)).astype(np.float32)
        audio[2, :4 * HOP] = 0.0
        _CACHE["audio"] = audio
    return _CACHE["audio"]


def _oracle(oracle_c, n_filters, nwin=400, audio=None, key=None):
    """(spec (n, F, ncols) of the oracle, its dB in NumPy, the calibration range chosen from that dB): the 20th and 80th
    percentile, so that the normalised values leave [0, 1] on both sides."""
    from oracle import ref_numpy
    key = key or ("oracle", n_filters, nwin)
    if key not in _CACHE:
        audio = _audio() if audio is None else audio
        coefs = ref_numpy.gammatone_coefs(16000, n_filters, 50)
        ncols = (audio.shape[1] - nwin) // HOP + 1
        spec = np.stack([oracle_c.gammatone_spec(a, coefs, nwin, HOP, ncols) for a in audio])
        db = 20 * np.log10(spec + 1e-9)
        lo, hi = (float(v) for v in np.percentile(db, (20, 80)))
        _CACHE[key] = (spec, db, (lo, hi))
    return _CACHE[key]


def _expected_raster(oracle_c, db_dev, db_range, thr=THR, gap=GAP):
    """NumPy's floor and normalisation of a dB array and the oracle's encoder, per stream: (n, F, ncols * n_thr)."""
    lo, hi = db_range
    norm = (np.maximum(db_dev, hi - 80) - lo) / (hi - lo + 1e-8)
    return np.stack([oracle_c.encode_hysteresis(x, thr, gap) for x in norm])


def _filled(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def _push_plan(torch, gs, audio, plan):
    """Push `audio` (n, samples) through `gs` as `plan` says (a list of per-push hop counts, an int for every stream or one
    per stream), into outputs pre-filled with 0xAA, behind every stream's samples a constant nobody may read.  Checks the
    counts, the fill behind them and that an idle stream's state block stays; returns the concatenated (raster, spec, db)
    per stream and the final state bytes."""
    from lsm_speech_classifier_amd import frontend
    n, n_thr, F, R = gs.n_streams, gs.n_thr, gs.n_filters, gs.redundancy
    done = np.zeros(n, dtype=np.int64)
    parts = [([], [], []) for _ in range(n)]
    for step in plan:
        new = np.full(n, step, dtype=np.int64) if np.ndim(step) == 0 else np.asarray(step, dtype=np.int64)
        H = max(int(new.max()), 1)
        chunk = np.full((n, H * HOP), 7.0, dtype=np.float32)
        for b in range(n):
            chunk[b, :new[b] * HOP] = audio[b, done[b] * HOP:(done[b] + new[b]) * HOP]
        raster = _filled(torch, (n, F * R, H * n_thr), torch.uint8)
        spec, db = _filled(torch, (n, F, H), torch.float64), _filled(torch, (n, F, H), torch.float64)
        before = gs.state.clone()
        want = frontend.stream_column_plan(gs.seen.copy(), new, gs.nwin, gs.hop)
        got_r, cols, got_db, got_spec = gs.push(chunk, new, raster_out=raster, db_out=db, spec_out=spec)
        torch.cuda.synchronize()
        assert got_r is raster and got_db is db and got_spec is spec
        assert cols.tolist() == want.tolist(), f"columns of push {new.tolist()}"
        r_h, s_h, d_h = raster.cpu().numpy(), spec.cpu().numpy(), db.cpu().numpy()
        for b in range(n):
            c = int(cols[b])
            assert (r_h[b, :, c * n_thr:] == FILL).all(), f"raster behind stream {b}'s {c} columns, push {new.tolist()}"
            assert (s_h[b, :, c:].view(np.uint8) == FILL).all() and (d_h[b, :, c:].view(np.uint8) == FILL).all()
            assert set(np.unique(r_h[b, :, :c * n_thr])) <= {0, 1}
            parts[b][0].append(r_h[b, :, :c * n_thr])
            parts[b][1].append(s_h[b, :, :c])
            parts[b][2].append(d_h[b, :, :c])
            if new[b] == 0:
                assert torch.equal(gs.state[b], before[b]), f"state block of idle stream {b}"
        done += new
    out = [tuple(np.concatenate(p, axis=1) for p in parts[b]) for b in range(n)]
    return out, gs.state.cpu().numpy()


def _uncut(torch, oracle_c, n_filters, nwin=400, redundancy=1, thr=THR, gap=GAP):
    """One push of all 40 hops (cached): (per-stream (raster, spec, db), final state, calibration range)."""
    from lsm_speech_classifier_amd import frontend
    key = ("uncut", n_filters, nwin, redundancy, tuple(thr), gap)
    if key not in _CACHE:
        _, _, db_range = _oracle(oracle_c, n_filters, nwin)
        gs = frontend.GammatoneStream(n_filters, N_STREAMS, db_range, thresholds=thr, gap=gap, redundancy=redundancy,
                                      nwin=nwin, hop=HOP)
        out, state = _push_plan(torch, gs, _audio(), [HOPS])
        _CACHE[key] = (out, state, db_range)
    return _CACHE[key]


def _check_against_oracle(oracle_c, out, n_filters, nwin, db_range, thr=THR, gap=GAP):
    spec_ref, db_ref, _ = _oracle(oracle_c, n_filters, nwin)
    ncols, n_thr = _ncols(nwin), len(thr)
    for b in range(N_STREAMS):
        raster, spec, db = out[b]
        assert spec.shape == (n_filters, ncols) and raster.shape == (n_filters, ncols * n_thr)
        np.testing.assert_array_equal(spec, spec_ref[b], err_msg=f"columns of stream {b}")
        err = np.abs(db - 20 * np.log10(spec + 1e-9)).max()
        print(f"F={n_filters} nwin={nwin} stream {b}: max |dB - 20 log10(spec + 1e-9)| = {err:.3e}")
        assert err <= 1e-12
    want = _expected_raster(oracle_c, np.stack([o[2] for o in out]), db_range, thr, gap)
    for b in range(N_STREAMS):
        for k in range(n_thr):
            plane = want[b][:, k::n_thr]
            assert plane.any() and not plane.all(), f"threshold plane {k} of stream {b} is constant: nothing is crossed"
        np.testing.assert_array_equal(out[b][0], want[b], err_msg=f"raster of stream {b}")
    return want


def _ragged_plan(seed):
    """Eight pushes per stream, zeros included, 40 hops in all for every stream."""
    rng = np.random.RandomState(seed)
    plan = np.zeros((8, N_STREAMS), dtype=np.int64)
    for b in range(N_STREAMS):
        cuts = np.sort(rng.randint(0, HOPS + 1, size=7))
        cuts[rng.randint(0, 7)] = cuts[rng.randint(0, 7)]               # (sorted again below) a repeated cut: a zero push
        cuts = np.concatenate([[0], np.sort(cuts), [HOPS]])
        plan[:, b] = np.diff(cuts)
    assert (plan.sum(axis=0) == HOPS).all() and (plan == 0).any()
    return [row for row in plan]


PLANS = {"1-1-1-37": [1, 1, 1, 37], "3-0-5-32": [3, 0, 5, 32], "20x2": [2] * 20, "ragged": _ragged_plan(5)}


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("n_filters", FILTERS)
def test_uncut_push_equals_the_oracle(torch_cuda, oracle_c, n_filters):
    out, _, db_range = _uncut(torch_cuda, oracle_c, n_filters)
    _check_against_oracle(oracle_c, out, n_filters, 400, db_range)
    # the floor is in use (stream 2's silent columns) and values leave [0, 1] on both sides
    db = np.stack([o[2] for o in out])
    lo, hi = db_range
    assert (db < hi - 80).any() and (db > hi).any() and ((db < lo) & (db > hi - 80)).any()


@pytest.mark.parametrize("plan", list(PLANS), ids=list(PLANS))
@pytest.mark.parametrize("n_filters", FILTERS)
def test_a_cut_run_equals_the_uncut_run(torch_cuda, oracle_c, n_filters, plan):
    from lsm_speech_classifier_amd import frontend
    out, state, db_range = _uncut(torch_cuda, oracle_c, n_filters)
    gs = frontend.GammatoneStream(n_filters, N_STREAMS, db_range, thresholds=THR, gap=GAP)
    cut, cut_state = _push_plan(torch_cuda, gs, _audio(), PLANS[plan])
    for b in range(N_STREAMS):
        for got, want, what in zip(cut[b], out[b], ("raster", "columns", "dB")):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what} of stream {b}, plan {plan}"
    assert cut_state.tobytes() == state.tobytes(), f"final state blocks, plan {plan}"
    assert gs.seen.tolist() == [HOPS] * N_STREAMS


def test_start_of_a_stream_and_reset(torch_cuda, oracle_c):
    """The first and the second hop of a stream complete no column, the third completes column 0; after reset(slot) that
    stream alone starts over."""
    from lsm_speech_classifier_amd import frontend
    F = 64
    out, _, db_range = _uncut(torch_cuda, oracle_c, F)
    audio = _audio()
    gs = frontend.GammatoneStream(F, N_STREAMS, db_range)
    assert not gs.state.any()
    got = [[] for _ in range(N_STREAMS)]

    def push(first_hop, hops):
        """Every stream's hops [first_hop[b], first_hop[b] + hops[b])."""
        H = max(max(hops), 1)
        chunk = np.zeros((N_STREAMS, H * HOP), dtype=np.float32)
        for b in range(N_STREAMS):
            chunk[b, :hops[b] * HOP] = audio[b, first_hop[b] * HOP:(first_hop[b] + hops[b]) * HOP]
        raster, cols = gs.push(chunk, np.asarray(hops))
        for b in range(N_STREAMS):
            got[b].append(raster[b, :, :cols[b] * 4].cpu().numpy())
        return cols.tolist()

    assert push([0, 0, 0], [1, 1, 1]) == [0, 0, 0]
    assert push([1, 1, 1], [1, 1, 1]) == [0, 0, 0]
    assert push([2, 2, 2], [1, 1, 1]) == [1, 1, 1]
    for b in range(N_STREAMS):
        np.testing.assert_array_equal(np.concatenate(got[b], axis=1), out[b][0][:, :4], err_msg=f"column 0 of stream {b}")
    assert push([3, 3, 3], [5, 5, 5]) == [5, 5, 5]
    gs.reset([1])
    assert not gs.state[1].any() and gs.state[0].any() and gs.state[2].any() and gs.seen.tolist() == [8, 0, 8]
    got[1] = []
    assert push([8, 0, 8], [2, 2, 2]) == [2, 0, 2]                      # a push of two hops into a fresh stream: nothing
    assert push([10, 2, 10], [30, 38, 30]) == [30, 38, 30]
    for b in range(N_STREAMS):
        np.testing.assert_array_equal(np.concatenate(got[b], axis=1), out[b][0], err_msg=f"stream {b}")


@pytest.mark.parametrize("nwin", [320, 160, 640])
def test_other_strides(torch_cuda, oracle_c, nwin):
    """One, two and four windows live at a time (the default has three): uncut against the oracle, cut against uncut."""
    from lsm_speech_classifier_amd import frontend
    F = 64
    out, state, db_range = _uncut(torch_cuda, oracle_c, F, nwin)
    assert out[0][1].shape[1] == {320: 39, 160: 40, 640: 37}[nwin]
    _check_against_oracle(oracle_c, out, F, nwin, db_range)
    for plan in ("1-1-1-37", "3-0-5-32", "ragged"):
        gs = frontend.GammatoneStream(F, N_STREAMS, db_range, nwin=nwin, hop=HOP)
        cut, cut_state = _push_plan(torch_cuda, gs, _audio(), PLANS[plan])
        for b in range(N_STREAMS):
            for got, want, what in zip(cut[b], out[b], ("raster", "columns", "dB")):
                assert got.tobytes() == want.tobytes(), f"{what} of stream {b}, nwin {nwin}, plan {plan}"
        assert cut_state.tobytes() == state.tobytes()


def test_latches_are_carried_over_a_push_boundary(torch_cuda, oracle_c):
    """Noise at one level for 20 hops, then 10 dB lower: with ON = 0.9 and OFF = 0.5 on a 40 dB range below the loud level a
    channel crosses ON while loud and then stays between the two bounds.  The push boundary (hop 30) lies inside the quiet
    part, so in the second push nothing crosses ON: the latch is on there only because it was carried.  THIS TEST FAILS IF
    THE LATCHES ARE RESET PER PUSH -- the second push's raster would be zeros in the channels picked below."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, thr, gap, cut = 32, [0.9], 0.4, 30
    rng = np.random.RandomState(77)
    n = HOPS * HOP
    x = rng.standard_normal(n) * 0.2
    x[n // 2:] *= 10.0 ** (-10.0 / 20.0)
    audio = x.astype(np.float32)[None]
    _, db_ref, _ = _oracle(oracle_c, F, audio=audio, key=("latch", F))
    hi = float(np.median(db_ref[0][:, 5:18]))
    lo = hi - 40.0
    # the precondition, on the oracle's dB: channels that crossed ON before the boundary and lie strictly between the
    # bounds in every column of the second push (columns 28..37); well inside, so that log10's last bit decides nothing
    norm = (np.maximum(db_ref[0], hi - 80) - lo) / (hi - lo + 1e-8)
    first_cols = _ncols(400, cut)
    held = (norm[:, :first_cols] > 0.91).any(axis=1) & (norm[:, first_cols - 8:] > 0.51).all(axis=1) \
        & (norm[:, first_cols - 8:] < 0.89).all(axis=1)
    assert held.sum() >= 4, f"only {held.sum()} channels hold their latch over the boundary"
    gs = frontend.GammatoneStream(F, 1, (lo, hi), thresholds=thr, gap=gap)
    r1, c1, db1, _ = gs.push(audio[:, :cut * HOP], want_db=True)
    r2, c2, db2, _ = gs.push(audio[:, cut * HOP:], want_db=True)
    assert c1.tolist() == [first_cols] and c2.tolist() == [HOPS - cut]
    second = r2[0, :, :int(c2[0])].cpu().numpy()
    assert second[held].all(), "a carried latch went off in the second push"
    db_dev = np.concatenate([db1[0, :, :int(c1[0])].cpu().numpy(), db2[0, :, :int(c2[0])].cpu().numpy()], axis=1)
    want = _expected_raster(oracle_c, db_dev[None], (lo, hi), thr, gap)[0]
    np.testing.assert_array_equal(np.concatenate([r1[0, :, :first_cols].cpu().numpy(), second], axis=1), want)
    # the oracle's encoder started afresh on the second push's columns leaves those channels off: the test discriminates
    afresh = _expected_raster(oracle_c, db_dev[None, :, first_cols:], (lo, hi), thr, gap)[0]
    assert not afresh[held].any()


def test_negative_gap_tables(torch_cuda, oracle_c):
    """The threshold tables of test_gpu_fused.py's negative-gap test (off above on: an active latch can see both
    comparisons true and is cleared), uncut against the oracle's encoder and cut against uncut."""
    from lsm_speech_classifier_amd import frontend
    F = 64
    rng = np.random.RandomState(4)
    for gap in (-0.05, -0.2):
        thr = sorted(rng.uniform(0.3, 0.95, size=4).tolist())
        out, _, db_range = _uncut(torch_cuda, oracle_c, F, thr=thr, gap=gap)
        want = _check_against_oracle(oracle_c, out, F, 400, db_range, thr, gap)
        on, off = frontend.threshold_tables(thr, gap, np.float64)
        assert (off > on).all() and want.any()
        gs = frontend.GammatoneStream(F, N_STREAMS, db_range, thresholds=thr, gap=gap)
        cut, _ = _push_plan(torch_cuda, gs, _audio(), PLANS["ragged"])
        for b in range(N_STREAMS):
            assert cut[b][0].tobytes() == out[b][0].tobytes(), f"stream {b}, gap {gap}"


def test_redundancy(torch_cuda, oracle_c):
    out1, _, _ = _uncut(torch_cuda, oracle_c, 65)
    out3, _, _ = _uncut(torch_cuda, oracle_c, 65, redundancy=3)
    for b in range(N_STREAMS):
        assert out3[b][0].shape == (3 * 65, _ncols(400) * 4)
        for c in range(3 * 65):
            assert out3[b][0][c].tobytes() == out1[b][0][c // 3].tobytes(), f"row {c} of stream {b}"
        assert out3[b][1].tobytes() == out1[b][1].tobytes()
    # three thresholds: rows that are no multiple of four bytes take the byte stores
    from lsm_speech_classifier_amd import frontend
    thr = [0.6, 0.8, 0.9]
    out, _, db_range = _uncut(torch_cuda, oracle_c, 65, redundancy=2, thr=thr)
    want = _expected_raster(oracle_c, np.stack([o[2] for o in out]), db_range, thr, GAP)
    for b in range(N_STREAMS):
        np.testing.assert_array_equal(out[b][0], np.repeat(want[b], 2, axis=0))


def test_refusals_launch_nothing(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    F, n, H = 64, 2, 4
    tab = frontend.gammatone_filter_table(16000, F, 50)
    coefs = torch.from_numpy(tab).cuda()
    audio = torch.zeros((n, H * HOP + 4), dtype=torch.float32, device="cuda")
    on, off = frontend.threshold_tables(THR, GAP, np.float64)
    nbytes = lib.lsm_gammatone_stream_state_bytes(F, 400, HOP)
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes >= F * (10 * 8 + 8)
    assert lib.lsm_gammatone_stream_state_bytes(1, 400, HOP) == 0 and lib.lsm_gammatone_stream_state_bytes(F, 641, HOP) == 0
    state = torch.full((n, nbytes + 16), 0x3C, dtype=torch.uint8, device="cuda")
    raster = torch.full((n, F, H * 4 + 4), FILL, dtype=torch.uint8, device="cuda")
    spec = torch.full((n, F, H + 1), -7.0, dtype=torch.float64, device="cuda")
    hops = torch.full((n + 1,), H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda x: C.c_void_p(x) if x else None

    def run(F=F, nwin=400, hop=HOP, H=H, lo=-60.0, hi=-10.0, a=audio.data_ptr(), k=coefs.data_ptr(), hp=hops.data_ptr(),
            s_in=state.data_ptr(), s_out=state.data_ptr(), r=raster.data_ptr(), sp=spec.data_ptr(), db=0, n_thr=4, red=1):
        return lib.lsm_gammatone_stream_f64(void(a), n, H, void(k), F, nwin, hop, void(hp), lo, hi,
                                            C.c_void_p(on.ctypes.data), C.c_void_p(off.ctypes.data), n_thr, red, void(s_in),
                                            void(s_out), void(r), void(sp), void(db), 3, stream)

    cases = [
        (lambda: run(F=1), "n_filters >= 2"), (lambda: run(nwin=641), "nwin=641"), (lambda: run(nwin=159), "nwin=159"),
        (lambda: run(H=0), "n_hops=0"), (lambda: run(H=-2), "n_hops"), (lambda: run(lo=-10.0, hi=-10.0), "db_lo < db_hi"),
        (lambda: run(lo=-10.0, hi=-60.0), "db_lo < db_hi"), (lambda: run(lo=float("nan")), "finite"),
        (lambda: run(hi=float("inf")), "finite"), (lambda: run(lo=float("-inf")), "finite"),
        (lambda: run(r=0), "raster_out is required"), (lambda: run(r=raster.data_ptr() + 2), "raster_out is misaligned"),
        (lambda: run(a=audio.data_ptr() + 2), "audio is misaligned"), (lambda: run(k=coefs.data_ptr() + 4), "coefs is misaligned"),
        (lambda: run(hp=hops.data_ptr() + 2), "stream_hops is misaligned"), (lambda: run(s_in=state.data_ptr() + 8), "state_in is misaligned"),
        (lambda: run(s_out=state.data_ptr() + 8), "state_out is misaligned"), (lambda: run(sp=spec.data_ptr() + 4), "spec_out is misaligned"),
        (lambda: run(db=spec.data_ptr() + 4), "db_out is misaligned"), (lambda: run(n_thr=0), "n_thr"), (lambda: run(n_thr=9), "n_thr"),
        (lambda: run(red=0), "redundancy"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        with pytest.raises(_lib.LsmHipError, match=words):
            _lib.check(rc, "refused")
    torch.cuda.synchronize()
    assert bool((raster == FILL).all()) and bool((spec == -7.0).all()) and bool((state == 0x3C).all()), \
        "a refused call wrote to its outputs"
    # the Python layer refuses before it calls the library
    with pytest.raises(ValueError, match="n_filters"):
        frontend.GammatoneStream(1, 2, (-60.0, -10.0))
    with pytest.raises(ValueError, match="db_range"):
        frontend.GammatoneStream(8, 2, (-10.0, -60.0))
    with pytest.raises(ValueError, match="nwin"):
        frontend.GammatoneStream(8, 2, (-60.0, -10.0), nwin=700)
    gs = frontend.GammatoneStream(8, 2, (-60.0, -10.0))
    for bad in ((5, 0), (0, -1), (1,), (1.0, 2.0)):
        with pytest.raises(ValueError, match="hops"):
            gs.push(np.zeros((2, 4 * HOP), dtype=np.float32), np.asarray(bad))
    with pytest.raises(ValueError, match="audio"):
        gs.push(np.zeros((2, 4 * HOP + 1), dtype=np.float32))
    assert gs.seen.tolist() == [0, 0] and not gs.state.any()


@pytest.mark.parametrize("n_filters", [3, 65])     # 3: 264 bytes in use + 8 of padding; 65: a second wave group with dead lanes
def test_separate_state_buffers(torch_cuda, n_filters):
    """`lsm_gammatone_stream_f64` with state_out != state_in, with no state_in and with no state_out, against its own
    in-place run: two pushes of H = 2 hops of which the streams deliver [2, 0, 1] (stream 1 is idle), nwin = 10 over
    hop = 4 (three live windows).  `GammatoneStream` only ever passes state_out = state_in."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    F, n, H, nwin, hop, R, PAD = n_filters, 3, 2, 10, 4, 2, 0x5A
    used = (10 * 8 + 8) * F                                     # 8 filter + 2 window doubles, latch and hop count per channel
    block = lib.lsm_gammatone_stream_state_bytes(F, nwin, hop)
    assert block == (used + 15) // 16 * 16 and block - used == 8
    tab = frontend.gammatone_filter_table(16000, F, 50)
    coefs, flags = torch.from_numpy(tab).cuda(), frontend.coef_flags(tab)
    on, off = frontend.threshold_tables(THR, GAP, np.float64)
    rng = np.random.RandomState(77 + F)
    pushes = [torch.from_numpy((rng.standard_normal((n, H * hop)) * 0.3).astype(np.float32)).cuda() for _ in range(2)]
    hops = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def push(audio, s_in, s_out):
        raster = torch.full((n, F * R, H * 4), FILL, dtype=torch.uint8, device="cuda")
        db = torch.full((n, F, H), -7.0, dtype=torch.float64, device="cuda")
        spec = torch.full((n, F, H), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.lsm_gammatone_stream_f64(
            C.c_void_p(audio.data_ptr()), n, H, C.c_void_p(coefs.data_ptr()), F, nwin, hop, C.c_void_p(hops.data_ptr()),
            -40.0, -8.0, C.c_void_p(on.ctypes.data), C.c_void_p(off.ctypes.data), 4, R,
            C.c_void_p(s_in.data_ptr()) if s_in is not None else None,
            C.c_void_p(s_out.data_ptr()) if s_out is not None else None, C.c_void_p(raster.data_ptr()),
            C.c_void_p(spec.data_ptr()), C.c_void_p(db.data_ptr()), flags, stream), "lsm_gammatone_stream_f64")
        torch.cuda.synchronize()
        return raster, db, spec

    def same(a, b):
        return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))

    start = torch.zeros((n, block), dtype=torch.uint8, device="cuda")
    start[:, used:] = PAD
    # the in-place run
    st = start.clone()
    out1 = push(pushes[0], st, st)
    st1 = st.clone()
    out2 = push(pushes[1], st, st)
    assert bool((out2[2][0] > 0).all()) and bool((out2[0][1:] == FILL).all())      # stream 0's fourth hop closes columns
    assert torch.equal(st1[1], start[1]) and torch.equal(st[1], start[1]) and not torch.equal(st1[0], start[0])
    # (a) - (d) out of place, state_out pre-filled
    s0, s1, s2 = start.clone(), torch.full_like(start, 0x3C), torch.full_like(start, 0x3C)
    assert same(push(pushes[0], s0, s1), out1), "out of place: other outputs than in place"
    assert torch.equal(s1[:, :used], st1[:, :used]), "out of place: other state bytes than in place"
    assert torch.equal(s0, start), "state_in was written"
    assert torch.equal(s1[1], start[1]), "the idle stream's block did not arrive as it was"
    assert bool((s1[[0, 2], used:] == PAD).all()), "the padding of the active streams did not travel"
    assert same(push(pushes[1], s1, s2), out2) and torch.equal(s2, st), "second push out of place"
    assert torch.equal(s1[:, :used], st1[:, :used]), "state_in was written"
    # (e) no state_in: a block of zeros
    zeros, s3, s4 = torch.zeros_like(start), torch.full_like(start, 0x3C), torch.full_like(start, 0x3C)
    assert same(push(pushes[0], None, s3), push(pushes[0], zeros, s4)) and torch.equal(s3, s4)
    assert not s3[1].any() and torch.equal(s3[:, :used], st1[:, :used])
    # (f) no state_out: the same raster, no state written
    assert same(push(pushes[1], s1, None), out2) and torch.equal(s1[:, :used], st1[:, :used])
    assert bool((s1[[0, 2], used:] == PAD).all())


def test_db_range_is_the_split_paths_floored_range(torch_cuda, oracle_c):
    from lsm_speech_classifier_amd import frontend, synth
    from oracle import ref_numpy
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    clips = synth.class_chirps([0, 3, 7], seed=12)
    clips[1] *= 1e-6                                                    # far below: the 80 dB floor decides the lower bound
    lo, hi = fe.db_range(clips)
    coefs = ref_numpy.gammatone_coefs(16000, 16, 50)
    db = 20 * np.log10(np.stack([oracle_c.gammatone_spec(a, coefs, fe.nwin, fe.hop, fe.ncols) for a in clips]) + 1e-9)
    assert abs(hi - db.max()) <= 1e-12 and db.min() < db.max() - 80 and lo == hi - 80.0
    lo2, hi2 = fe.db_range(clips[2:])
    assert abs(hi2 - db[2].max()) <= 1e-12 and abs(lo2 - max(db[2].min(), db[2].max() - 80)) <= 1e-12
    with pytest.raises(ValueError, match="mel"):
        frontend.SpikeFrontEnd(16, "mel").db_range(clips)


def test_audio_stream_bank_end_to_end(torch_cuda, oracle_c):
    """Audio in, sliding-window rows out: ragged pushes through AudioStreamBank equal StreamBank fed with the uncut raster of
    the first test in one push, and the oracle's feature rows on slices of the oracle's spike matrix of that raster."""
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn
    F, S, K, H = 64, 8, 3, 1
    out, _, db_range = _uncut(torch, oracle_c, F)
    steps = _ncols(400) * 4
    G = steps // S
    assert steps == 152 and G == 19
    uncut = np.stack([o[0] for o in out])
    res = R.build_reservoir(R.SimulationParams(num_neurons=200, num_output_neurons=40, small_world_graph_k=40,
                                               mean_weight=2.0 / 20, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    bank = pipeline.StreamBank(net, N_STREAMS, S, K, H, ALL_KEYS)
    want, want_counts = bank.push(uncut[:, :, :G * S], [G] * N_STREAMS)
    assert want_counts.tolist() == [G - K + 1] * N_STREAMS
    want = want[:, :G - K + 1].cpu().numpy()
    burst = int(res.burst_isi_max)
    for b in range(N_STREAMS):
        sm = oracle_c.lif_run(res, uncut[b][:, :G * S], ALL_KEYS)[1]
        assert sm[:, res.out_idx].any(), f"the reservoir's output neurons stay silent on stream {b}"
        for w in range(G - K + 1):
            np.testing.assert_array_equal(want[b, w], ref_numpy.feature_row(sm[w * H * S:(w * H + K) * S], res.out_idx, burst,
                                                                            ALL_KEYS), err_msg=f"stream {b}, window {w}")
    gs = frontend.GammatoneStream(F, N_STREAMS, db_range)
    abank = pipeline.AudioStreamBank(gs, net, S, K, H, ALL_KEYS)
    audio = _audio()
    done = np.zeros(N_STREAMS, dtype=np.int64)
    got = [[] for _ in range(N_STREAMS)]
    emitted = np.zeros(N_STREAMS, dtype=np.int64)
    for new in _ragged_plan(9):
        Hh = max(int(new.max()), 1)
        chunk = np.full((N_STREAMS, Hh * HOP), 7.0, dtype=np.float32)
        for b in range(N_STREAMS):
            chunk[b, :new[b] * HOP] = audio[b, done[b] * HOP:(done[b] + new[b]) * HOP]
        rows, counts = abank.push(chunk, new)
        done += new
        # columns so far -> steps -> segments -> windows
        segs = frontend.stream_column_plan(0, done) * 4 // S
        total = np.where(segs >= K, (segs - K) // H + 1, 0)
        assert counts.tolist() == (total - emitted).tolist(), f"counts after {done.tolist()} hops"
        emitted = total
        for b in range(N_STREAMS):
            got[b].append(rows[b, :counts[b]].cpu().numpy())
            assert not rows[b, counts[b]:].any()
    for b in range(N_STREAMS):
        rows_b = np.concatenate(got[b])
        assert rows_b.shape == want[b].shape and rows_b.tobytes() == want[b].tobytes(), f"stream {b}"
    # a stream ends, a new one takes its slot: both halves and the pending columns start over
    abank.reset([2])
    assert not gs.state[2].any() and abank.pending_steps[2] == 0 and abank.bank.seen.tolist()[2] == 0
    chunk = np.zeros((N_STREAMS, HOPS * HOP), dtype=np.float32)
    chunk[2] = audio[2]
    rows, counts = abank.push(chunk, np.array([0, 0, HOPS]))
    assert counts.tolist() == [0, 0, G - K + 1]
    assert rows[2, :counts[2]].cpu().numpy().tobytes() == want[2].tobytes()
