"""Adaptive normalisation range for the streamed front ends (SPEC.md 1.9, include/lsm_hip_adaptive.h:
`lsm_adaptive_encode_f64` / `_f32`, `frontend.AdaptiveEncoder`, `frontend.AdaptiveStream`, through `pipeline.AudioStreamBank`).

The reference is the NumPy restatement of SPEC.md 1.9 (tests/adaptive_restatement.py, anchored to the pinned per-clip code
in test_adaptive_host.py) followed by the plain-C oracle's `encode_hysteresis`, bit for bit: on synthetic dB arrays, and end
to end on the DEVICE's dB array, so that no libm stands between the two sides.  A cut run is compared with the uncut one byte
for byte, ranges and state blocks included.  The code under test is never its own reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adaptive_restatement as A  # noqa: E402

pytestmark = pytest.mark.gpu

HOP, HOPS, N_STREAMS, COLS = 160, 40, 3, 60
THR4, THR3, GAP = [0.70, 0.80, 0.90, 0.95], [0.6, 0.8, 0.9], 0.1
FILL = 0xAA
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


def _tdtype(torch, dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


# ---- synthetic dB arrays and their expected outputs ------------------------------------------------------------------------
def _synthetic(dtype, F, cols=COLS):
    """(3, F, cols) dB values on a grid of 0.5 dB over 120 dB (exact in both types), so that equal extrema, repeated values
    and windows wider than the 80 dB floor all occur.  Stream 0: a level that wanders over 90 dB under a 30 dB spread;
    stream 1: the whole 120 dB everywhere, and ten identical columns (20..29) constant across filters; stream 2: like
    stream 0 with scattered NaNs and one column (33) that is NaN in every filter."""
    key = ("db", np.dtype(dtype).name, F, cols)
    if key not in _CACHE:
        rng = np.random.RandomState(1000 + F + cols)
        db = np.empty((N_STREAMS, F, cols), dtype=np.float64)
        for b in (0, 2):
            level = -100.0 + 0.5 * np.clip(np.cumsum(rng.randint(-24, 25, size=cols)) + 90, 0, 180)
            db[b] = level[None, :] + 0.5 * rng.randint(0, 61, size=(F, cols))
        db[1] = -100.0 + 0.5 * rng.randint(0, 241, size=(F, cols))
        db[1, :, 20:30] = -40.0
        nan = rng.rand(F, cols) < 0.05
        nan[:, 33] = True
        db[2][nan] = np.nan
        db = db.astype(dtype)
        assert (db[~np.isnan(db)] * 2 == np.round(db[~np.isnan(db)] * 2)).all()
        _CACHE[key] = db
    return _CACHE[key]


def _restated(dtype, F, L, cols=COLS):
    """Per stream (norm, lo, hi) of the restatement, computed once per (dtype, F, L, cols)."""
    key = ("norm", np.dtype(dtype).name, F, L, cols)
    if key not in _CACHE:
        _CACHE[key] = [A.adaptive(x, L) for x in _synthetic(dtype, F, cols)]
    return _CACHE[key]


def _expected(oracle_c, dtype, F, L, thr, gap, R, cols=COLS):
    """(raster (3, F * R, cols * n_thr), lo (3, cols), hi (3, cols)): the restatement and the oracle's encoder."""
    rest = _restated(dtype, F, L, cols)
    raster = np.stack([np.repeat(oracle_c.encode_hysteresis(norm, thr, gap), R, axis=0) for norm, _, _ in rest])
    return raster, np.stack([r[1] for r in rest]), np.stack([r[2] for r in rest])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- (a) the encoder alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 7, 100])
@pytest.mark.parametrize("F", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_encoder_equals_the_restatement_and_the_oracles_encoder(torch_cuda, oracle_c, dtype, F, L):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    db = _synthetic(dtype, F)
    rest = _restated(dtype, F, L)
    if L <= 7:
        assert not rest[1][0][:, 20 + L - 1:30].any() and (rest[1][1][26:30] == rest[1][2][26:30]).all()    # flat windows
    if F > 1:
        assert any(((hi - lo) == 80).any() for _, lo, hi in rest) or L < 7      # the floor decides a range
    for thr in (THR4, THR3):                                        # the word and the byte stores
        for R in (1, 2):
            want, want_lo, want_hi = _expected(oracle_c, dtype, F, L, thr, GAP, R)
            enc = frontend.AdaptiveEncoder(F, N_STREAMS, _tdtype(torch, dtype), L, thresholds=thr, gap=GAP, redundancy=R)
            assert enc.n_thr == len(thr) and enc.n_channels == F * R and not enc.state.any()
            raster, lo, hi = enc.push_db(torch.from_numpy(db).cuda(), want_range=True)
            torch.cuda.synchronize()
            what = f"{np.dtype(dtype).name} F={F} L={L} n_thr={len(thr)} R={R}"
            # the range first: a failure says whether the range or the latch is wrong
            assert _same(hi.cpu().numpy(), want_hi), f"hi, {what}"
            assert _same(lo.cpu().numpy(), want_lo), f"lo, {what}"
            np.testing.assert_array_equal(raster.cpu().numpy(), want, err_msg=f"raster, {what}")
    if F >= 64 and L >= 7:
        assert want.any() and not want.all()


def test_negative_gap(torch_cuda, oracle_c):
    """Off-thresholds above their on-thresholds: a value between them flips the latch (the bit-by-bit path)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, L, gap = 65, 7, -0.15
    thr = [0.35, 0.5, 0.65, 0.8]
    for dtype in (np.float64, np.float32):
        on, off = frontend.threshold_tables(thr, gap, dtype)
        assert (off > on).all()
        want, want_lo, want_hi = _expected(oracle_c, dtype, F, L, thr, gap, 1)
        enc = frontend.AdaptiveEncoder(F, N_STREAMS, _tdtype(torch, dtype), L, thresholds=thr, gap=gap)
        raster, lo, hi = enc.push_db(torch.from_numpy(_synthetic(dtype, F)).cuda(), want_range=True)
        assert _same(lo.cpu().numpy(), want_lo) and _same(hi.cpu().numpy(), want_hi)
        np.testing.assert_array_equal(raster.cpu().numpy(), want)
        norm = np.stack([r[0] for r in _restated(dtype, F, L)])
        assert ((norm > on[-1]) & (norm < off[-1])).any() and want.any() and not want.all()


@pytest.mark.parametrize("F,cols,L", [(65, 150, 7), (65, 150, 100), (5, 400, 300), (3, 129, 64), (3, 128, 65)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_more_columns_than_a_chunk(torch_cuda, oracle_c, dtype, F, cols, L):
    """A push of more than 64 columns walks them in chunks, the extrema carried from chunk to chunk in LDS (more than 256
    of them with L = 300); pushed in pieces that end inside, at and behind a chunk the outputs and the state are the same."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    db = torch.from_numpy(_synthetic(dtype, F, cols)).cuda()
    want, want_lo, want_hi = _expected(oracle_c, dtype, F, L, THR4, GAP, 1, cols)
    enc = frontend.AdaptiveEncoder(F, N_STREAMS, _tdtype(torch, dtype), L)
    raster, lo, hi = enc.push_db(db, want_range=True)
    assert _same(hi.cpu().numpy(), want_hi) and _same(lo.cpu().numpy(), want_lo)
    np.testing.assert_array_equal(raster.cpu().numpy(), want)
    cut = frontend.AdaptiveEncoder(F, N_STREAMS, _tdtype(torch, dtype), L)
    parts, pos = [], 0
    for n in (63, 1, 64, cols - 128):
        if n == 0:
            continue
        parts.append(cut.push_db(db[:, :, pos:pos + n].contiguous()).cpu().numpy())
        pos += n
    assert _same(np.concatenate(parts, axis=2), want)
    assert torch.equal(cut.state, enc.state)


# ---- (b) cuts, through the C ABI ---------------------------------------------------------------------------------------------
def _filled(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def _run_plan(torch, dtype, F, L, plan, thr=THR4, R=1, in_place=True):
    """The synthetic streams pushed through `lsm_adaptive_encode_*` as `plan` says (a list of per-push column counts, an int
    for every stream or one per stream), into outputs pre-filled with 0xAA, behind every stream's columns a constant nobody
    may read.  Checks the fill behind them and that an idle stream's state block stays; returns per stream the concatenated
    (raster, lo, hi) and the final state bytes."""
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    tdt = _tdtype(torch, dtype)
    fn = lib.lsm_adaptive_encode_f64 if dtype == np.float64 else lib.lsm_adaptive_encode_f32
    db_all = _synthetic(dtype, F)
    on, off = frontend.threshold_tables(thr, GAP, dtype)
    n_thr = len(on)
    nbytes = lib.lsm_adaptive_state_bytes(F, L, np.dtype(dtype).itemsize)
    state = torch.zeros((N_STREAMS, nbytes), dtype=torch.uint8, device="cuda")
    done = np.zeros(N_STREAMS, dtype=np.int64)
    parts = [([], [], []) for _ in range(N_STREAMS)]
    stream = torch.cuda.current_stream().cuda_stream
    for step in plan:
        new = np.full(N_STREAMS, step, dtype=np.int64) if np.ndim(step) == 0 else np.asarray(step, dtype=np.int64)
        H = max(int(new.max()), 1)
        chunk = np.full((N_STREAMS, F, H), 7.0, dtype=dtype)
        for b in range(N_STREAMS):
            chunk[b, :, :new[b]] = db_all[b, :, done[b]:done[b] + new[b]]
        d_db = torch.from_numpy(chunk).cuda()
        counts = torch.from_numpy(new.astype(np.int32)).cuda()
        raster = _filled(torch, (N_STREAMS, F * R, H * n_thr), torch.uint8)
        lo, hi = _filled(torch, (N_STREAMS, H), tdt), _filled(torch, (N_STREAMS, H), tdt)
        before = state.clone()
        target = state if in_place else _filled(torch, tuple(state.shape), torch.uint8)
        _lib.check(fn(C.c_void_p(d_db.data_ptr()), N_STREAMS, H, F, C.c_void_p(counts.data_ptr()), L,
                      C.c_void_p(on.ctypes.data), C.c_void_p(off.ctypes.data), n_thr, R, C.c_void_p(state.data_ptr()),
                      C.c_void_p(target.data_ptr()), C.c_void_p(raster.data_ptr()), C.c_void_p(lo.data_ptr()),
                      C.c_void_p(hi.data_ptr()), stream), "lsm_adaptive_encode")
        torch.cuda.synchronize()
        if not in_place:
            assert torch.equal(state, before), "an out-of-place call changed state_in"
        state = target
        r_h, lo_h, hi_h = raster.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
        for b in range(N_STREAMS):
            c = int(new[b])
            assert (r_h[b, :, c * n_thr:] == FILL).all(), f"raster behind stream {b}'s {c} columns, push {new.tolist()}"
            assert (lo_h[b, c:].view(np.uint8) == FILL).all() and (hi_h[b, c:].view(np.uint8) == FILL).all()
            assert set(np.unique(r_h[b, :, :c * n_thr])) <= {0, 1}
            parts[b][0].append(r_h[b, :, :c * n_thr])
            parts[b][1].append(lo_h[b, :c])
            parts[b][2].append(hi_h[b, :c])
            if c == 0:
                assert torch.equal(state[b], before[b]), f"state block of idle stream {b}"
        done += new
    assert done.tolist() == [COLS] * N_STREAMS
    out = [(np.concatenate(p[0], axis=1), np.concatenate(p[1]), np.concatenate(p[2])) for p in parts]
    return out, state.cpu().numpy()


PLANS = {"one-at-a-time": [1] * COLS, "0-3-37-20": [0, 3, 37, 20],
         "per-stream": [(5, 0, 60), (55, 20, 0), (0, 40, 0)]}


@pytest.mark.parametrize("L", [1, 7, 100])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_cut_run_equals_the_uncut_run(torch_cuda, oracle_c, dtype, L):
    torch = torch_cuda
    F = 65
    uncut, state = _run_plan(torch, dtype, F, L, [COLS])
    want, want_lo, want_hi = _expected(oracle_c, dtype, F, L, THR4, GAP, 1)
    for b in range(N_STREAMS):
        assert _same(uncut[b][0], want[b]) and _same(uncut[b][1], want_lo[b]) and _same(uncut[b][2], want_hi[b]), b
    assert state.any()
    for name, plan in PLANS.items():
        cut, cut_state = _run_plan(torch, dtype, F, L, plan)
        for b in range(N_STREAMS):
            for got, ref, what in zip(cut[b], uncut[b], ("raster", "lo", "hi")):
                assert _same(got, ref), f"{what} of stream {b}, plan {name}"
        assert cut_state.tobytes() == state.tobytes(), f"final state blocks, plan {name}"
    # out of place: the same outputs and the same final blocks, state_in untouched
    for name in ("0-3-37-20", "per-stream"):
        cut, cut_state = _run_plan(torch, dtype, F, L, PLANS[name], in_place=False)
        for b in range(N_STREAMS):
            assert _same(cut[b][0], uncut[b][0]), f"raster of stream {b}, plan {name}, out of place"
        assert cut_state.tobytes() == state.tobytes(), f"final state blocks, plan {name}, out of place"


def test_cuts_with_three_thresholds_and_redundancy(torch_cuda, oracle_c):
    torch = torch_cuda
    for dtype in (np.float64, np.float32):
        uncut, state = _run_plan(torch, dtype, 64, 7, [COLS], thr=THR3, R=2)
        want, _, _ = _expected(oracle_c, dtype, 64, 7, THR3, GAP, 2)
        cut, cut_state = _run_plan(torch, dtype, 64, 7, PLANS["per-stream"], thr=THR3, R=2)
        for b in range(N_STREAMS):
            assert _same(uncut[b][0], want[b]) and _same(cut[b][0], want[b]), b
        assert cut_state.tobytes() == state.tobytes()


def test_encoder_reset(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, L = 64, 7
    db = torch.from_numpy(_synthetic(np.float64, F)).cuda()
    want, _, _ = _expected(oracle_c, np.float64, F, L, THR4, GAP, 1)
    enc = frontend.AdaptiveEncoder(F, N_STREAMS, torch.float64, L)
    enc.push_db(db[:, :, :25].contiguous())
    enc.reset([1])
    assert not enc.state[1].any() and enc.state[0].any() and enc.state[2].any()
    chunk = db[:, :, 25:].clone()
    chunk[1] = db[1, :, :35]
    raster = enc.push_db(chunk).cpu().numpy()
    assert _same(raster[0], want[0][:, 100:]) and _same(raster[2], want[2][:, 100:])
    assert _same(raster[1], want[1][:, :140]), "a reset stream starts over"
    with pytest.raises(ValueError, match="slots"):
        enc.reset([3])


# ---- (c) refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_refusals_launch_nothing(torch_cuda, dtype):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    fn = lib.lsm_adaptive_encode_f64 if dtype == np.float64 else lib.lsm_adaptive_encode_f32
    tdt, elem = _tdtype(torch, dtype), np.dtype(dtype).itemsize
    F, n, H, L = 64, 2, 4, 7
    on, off = frontend.threshold_tables(THR4, GAP, dtype)
    nbytes = lib.lsm_adaptive_state_bytes(F, L, elem)
    db = torch.zeros((n, F, H + 1), dtype=tdt, device="cuda")
    state = torch.full((n, nbytes + 16), 0x3C, dtype=torch.uint8, device="cuda")
    raster = torch.full((n, F, H * 4 + 4), FILL, dtype=torch.uint8, device="cuda")
    rng_out = torch.full((2, n, H + 1), -7.0, dtype=tdt, device="cuda")
    cols = torch.full((n + 1,), H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda x: C.c_void_p(x) if x else None

    def run(n=n, F=F, H=H, L=L, d=db.data_ptr(), cp=cols.data_ptr(), t_on=on.ctypes.data, t_off=off.ctypes.data, n_thr=4,
            red=1, s_in=state.data_ptr(), s_out=state.data_ptr(), r=raster.data_ptr(), lo=rng_out[0].data_ptr(),
            hi=rng_out[1].data_ptr()):
        return fn(void(d), n, H, F, void(cp), L, void(t_on), void(t_off), n_thr, red, void(s_in), void(s_out), void(r),
                  void(lo), void(hi), stream)

    half = elem // 2
    cases = [
        (lambda: run(F=0), "n_filters=0"), (lambda: run(F=-1), "n_filters"), (lambda: run(L=0), "window_cols=0"),
        (lambda: run(L=4097), "window_cols=4097"), (lambda: run(H=0), "n_cols=0"), (lambda: run(H=-3), "n_cols"),
        (lambda: run(n=-1), "n_streams"), (lambda: run(n_thr=0), "n_thr=0"), (lambda: run(n_thr=9), "n_thr=9"),
        (lambda: run(red=0), "redundancy"), (lambda: run(t_on=0), "null threshold table"),
        (lambda: run(t_off=0), "null threshold table"), (lambda: run(r=0), "raster_out is required"),
        (lambda: run(d=0), "null db"),
        (lambda: run(r=raster.data_ptr() + 2), "raster_out is misaligned"),
        (lambda: run(cp=cols.data_ptr() + 2), "stream_cols is misaligned"),
        (lambda: run(d=db.data_ptr() + half), "db is misaligned"),
        (lambda: run(lo=rng_out[0].data_ptr() + half), "lo_out is misaligned"),
        (lambda: run(hi=rng_out[1].data_ptr() + half), "hi_out is misaligned"),
        (lambda: run(s_in=state.data_ptr() + 8), "state_in is misaligned"),
        (lambda: run(s_out=state.data_ptr() + 8), "state_out is misaligned"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        with pytest.raises(_lib.LsmHipError, match=words):
            _lib.check(rc, "refused")
    assert run(n=0) == 0                                                # no stream: nothing to do
    torch.cuda.synchronize()
    assert bool((raster == FILL).all()) and bool((rng_out == -7.0).all()) and bool((state == 0x3C).all()), \
        "a refused call wrote to its outputs"
    # the Python layer refuses before it calls the library
    for kwargs, words in (({"n_filters": 0}, "n_filters"), ({"window_cols": 0}, "window_cols"),
                          ({"window_cols": 4097}, "window_cols"), ({"redundancy": 0}, "redundancy"),
                          ({"n_streams": 0}, "n_streams"), ({"dtype": torch.float16}, "dtype")):
        args = {"n_filters": 8, "n_streams": 2, "dtype": tdt, **kwargs}
        with pytest.raises(ValueError, match=words):
            frontend.AdaptiveEncoder(**args)
    enc = frontend.AdaptiveEncoder(8, 2, tdt, 7)
    good = torch.zeros((2, 8, 4), dtype=tdt, device="cuda")
    for bad in (good[:, :4], good[:1], good.to(torch.float16), good[:, :, :0]):
        with pytest.raises(ValueError, match="db must be"):
            enc.push_db(bad)
    for bad in ((5, 0), (0, -1), (1,), (1.0, 2.0)):
        with pytest.raises(ValueError, match="cols"):
            enc.push_db(good, np.asarray(bad))
    with pytest.raises(ValueError, match="raster_out"):
        enc.push_db(good, raster_out=torch.zeros((2, 8, 15), dtype=torch.uint8, device="cuda"))
    assert not enc.state.any()
    with pytest.raises(ValueError, match="streamed front end"):
        frontend.AdaptiveStream(object())


# ---- (d), (e) end to end -------------------------------------------------------------------------------------------------------
def _audio():
    """3 streams of 40 hops of seeded noise under a level ramp of 50 dB up and down again (its peak at another place in
    every stream); stream 2 starts with four hops of exact silence."""
    if "audio" not in _CACHE:
        rng = np.random.RandomState(20261)
        n = HOPS * HOP
        t = np.arange(n) / n
        audio = np.empty((N_STREAMS, n), dtype=np.float32)
        for b, peak in enumerate((0.5, 0.35, 0.65)):
            level_db = -50.0 * np.abs(t - peak) / max(peak, 1 - peak)
            audio[b] = (rng.standard_normal(n) * 0.3 * 10.0 ** (level_db / 20.0)).astype(np.float32)
        audio[2, :4 * HOP] = 0.0
        _CACHE["audio"] = audio
    return _CACHE["audio"]


def _ragged_plan(seed):
    """Eight pushes per stream, zeros included, 40 hops in all for every stream."""
    rng = np.random.RandomState(seed)
    plan = np.zeros((8, N_STREAMS), dtype=np.int64)
    for b in range(N_STREAMS):
        cuts = np.sort(rng.randint(0, HOPS + 1, size=7))
        cuts[rng.randint(0, 7)] = cuts[rng.randint(0, 7)]
        plan[:, b] = np.diff(np.concatenate([[0], np.sort(cuts), [HOPS]]))
    assert (plan.sum(axis=0) == HOPS).all() and (plan == 0).any()
    return [row for row in plan]


AUDIO_PLANS = {"1-1-1-37": [1, 1, 1, 37], "3-0-5-32": [3, 0, 5, 32], "ragged": _ragged_plan(5)}


def _make_inner(kind, F, redundancy=1):
    from lsm_speech_classifier_amd import frontend
    if kind == "gammatone":
        return frontend.GammatoneStream(F, N_STREAMS, (-60.0, -10.0), redundancy=redundancy)   # the range: a placeholder
    return frontend.MelStream(F, N_STREAMS, (-60.0, -10.0), redundancy=redundancy)


def _push_audio(torch, ads, plan):
    """`_audio()` pushed through an AdaptiveStream as `plan` says, rasters pre-filled with 0xAA; returns per stream the
    concatenated (raster, dB) and both final states."""
    audio = _audio()
    n, n_thr = ads.n_streams, ads.n_thr
    done = np.zeros(n, dtype=np.int64)
    parts = [([], []) for _ in range(n)]
    for step in plan:
        new = np.full(n, step, dtype=np.int64) if np.ndim(step) == 0 else np.asarray(step, dtype=np.int64)
        H = max(int(new.max()), 1)
        chunk = np.full((n, H * HOP), 7.0, dtype=np.float32)
        for b in range(n):
            chunk[b, :new[b] * HOP] = audio[b, done[b] * HOP:(done[b] + new[b]) * HOP]
        raster = _filled(torch, (n, ads.n_channels, H * n_thr), torch.uint8)
        got, cols, db = ads.push(chunk, new, raster_out=raster, want_db=True)
        torch.cuda.synchronize()
        assert got is raster and tuple(db.shape) == (n, ads.n_filters, H) and db.dtype == ads.db_dtype
        r_h, d_h = raster.cpu().numpy(), db.cpu().numpy()
        for b in range(n):
            c = int(cols[b])
            assert (r_h[b, :, c * n_thr:] == FILL).all(), f"raster behind stream {b}'s {c} columns, push {new.tolist()}"
            parts[b][0].append(r_h[b, :, :c * n_thr])
            parts[b][1].append(d_h[b, :, :c])
        done += new
    assert ads.seen.tolist() == [HOPS] * n
    out = [(np.concatenate(p[0], axis=1), np.concatenate(p[1], axis=1)) for p in parts]
    return out, ads.inner.state.cpu().numpy(), ads.encoder.state.cpu().numpy()


def _uncut_audio(torch, kind, F):
    from lsm_speech_classifier_amd import frontend
    key = ("uncut", kind, F)
    if key not in _CACHE:
        _CACHE[key] = _push_audio(torch, frontend.AdaptiveStream(_make_inner(kind, F), 100), [HOPS])
    return _CACHE[key]


@pytest.mark.parametrize("kind,F", [("gammatone", 2), ("gammatone", 65), ("mel", 40)])
def test_adaptive_stream_end_to_end(torch_cuda, oracle_c, kind, F):
    """The raster is the restatement of the DEVICE's dB columns and the oracle's encoder; cut pushes equal the uncut push
    byte for byte, both states included; the wrapper carries what AudioStreamBank asks of a front end."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    out, inner_state, enc_state = _uncut_audio(torch, kind, F)
    ncols = HOPS - 2 if kind == "gammatone" else HOPS - 7 + 1       # stream_column_plan / mel_stream_frame_plan of 40 hops
    dtype = np.float64 if kind == "gammatone" else np.float32
    for b in range(N_STREAMS):
        raster, db = out[b]
        assert db.dtype == dtype and db.shape == (F, ncols) and raster.shape == (F, ncols * 4)
        norm, _, _ = A.adaptive(db, 100)
        want = oracle_c.encode_hysteresis(norm, THR4, GAP)
        assert want.any() and not want.all(), f"stream {b}: nothing is crossed"
        np.testing.assert_array_equal(raster, want, err_msg=f"raster of stream {b}")
    ads = frontend.AdaptiveStream(_make_inner(kind, F), 100)
    assert ads.streamed is True and ads.filterbank == kind and ads.hop == HOP and ads.n_thr == 4 and ads.redundancy == 1
    assert (ads.n_filters, ads.n_streams, ads.n_channels) == (F, N_STREAMS, F) and ads.device == ads.inner.device
    assert ads.seen is ads.inner.seen
    for name, plan in AUDIO_PLANS.items():
        ads = frontend.AdaptiveStream(_make_inner(kind, F), 100)
        cut, cut_inner, cut_enc = _push_audio(torch, ads, plan)
        for b in range(N_STREAMS):
            assert _same(cut[b][0], out[b][0]), f"raster of stream {b}, plan {name}"
            assert _same(cut[b][1], out[b][1]), f"dB of stream {b}, plan {name}"
        assert cut_inner.tobytes() == inner_state.tobytes(), f"front end's final state, plan {name}"
        assert cut_enc.tobytes() == enc_state.tobytes(), f"encoder's final state, plan {name}"


def test_a_short_window_and_redundancy_end_to_end(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, L = 16, 7
    ads = frontend.AdaptiveStream(_make_inner("gammatone", F, redundancy=2), L)
    out, _, _ = _push_audio(torch, ads, AUDIO_PLANS["ragged"])
    for b in range(N_STREAMS):
        raster, db = out[b]
        want = np.repeat(oracle_c.encode_hysteresis(A.adaptive(db, L)[0], THR4, GAP), 2, axis=0)
        np.testing.assert_array_equal(raster, want, err_msg=f"stream {b}")


# ---- (f) through AudioStreamBank ----------------------------------------------------------------------------------------------
def test_audio_stream_bank_takes_the_adaptive_stream(torch_cuda, oracle_c):
    """Ragged pushes through AudioStreamBank(AdaptiveStream) equal one uncut push, equal StreamBank fed with the uncut
    adaptive raster, and a reset slot starts over while the others continue."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn
    F, S, K, Hs = 65, 8, 3, 1
    out, _, _ = _uncut_audio(torch, "gammatone", F)
    uncut = np.stack([o[0] for o in out])
    steps = uncut.shape[2]
    G = steps // S
    assert steps == 152 and G == 19
    res = R.build_reservoir(R.SimulationParams(num_neurons=64, num_output_neurons=16, small_world_graph_k=16,
                                               mean_weight=2.0 / 8, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    want, want_counts = pipeline.StreamBank(net, N_STREAMS, S, K, Hs, ALL_KEYS).push(uncut[:, :, :G * S], [G] * N_STREAMS)
    assert want_counts.tolist() == [G - K + 1] * N_STREAMS
    want = want[:, :G - K + 1].cpu().numpy()
    assert want.any()
    audio = _audio()

    def bank():
        return pipeline.AudioStreamBank(frontend.AdaptiveStream(_make_inner("gammatone", F), 100), net, S, K, Hs, ALL_KEYS)

    one = bank()
    rows, counts = one.push(audio)
    assert counts.tolist() == [G - K + 1] * N_STREAMS
    assert rows[:, :G - K + 1].cpu().numpy().tobytes() == want.tobytes(), "one uncut push"
    abank = bank()
    done = np.zeros(N_STREAMS, dtype=np.int64)
    got = [[] for _ in range(N_STREAMS)]
    for new in _ragged_plan(9):
        Hh = max(int(new.max()), 1)
        chunk = np.full((N_STREAMS, Hh * HOP), 7.0, dtype=np.float32)
        for b in range(N_STREAMS):
            chunk[b, :new[b] * HOP] = audio[b, done[b] * HOP:(done[b] + new[b]) * HOP]
        rows, counts = abank.push(chunk, new)
        done += new
        for b in range(N_STREAMS):
            got[b].append(rows[b, :counts[b]].cpu().numpy())
            assert not rows[b, counts[b]:].any()
    for b in range(N_STREAMS):
        rows_b = np.concatenate(got[b])
        assert rows_b.shape == want[b].shape and rows_b.tobytes() == want[b].tobytes(), f"stream {b}"
    # a stream ends, a new one takes its slot: every half and the pending columns start over, the others continue
    gs = abank.gt
    abank.reset([2])
    assert not gs.inner.state[2].any() and not gs.encoder.state[2].any() and gs.encoder.state[0].any()
    assert gs.seen.tolist() == [HOPS, HOPS, 0] and abank.pending_steps[2] == 0
    chunk = np.zeros((N_STREAMS, HOPS * HOP), dtype=np.float32)
    chunk[2] = audio[2]
    rows, counts = abank.push(chunk, np.array([0, 0, HOPS]))
    assert counts.tolist() == [0, 0, G - K + 1]
    assert rows[2, :counts[2]].cpu().numpy().tobytes() == want[2].tobytes()


def test_audio_stream_bank_with_a_resampler(torch_cuda):
    """48 kHz PCM -> ResampleStream -> AdaptiveStream -> StreamBank: units cut two ways give the same rows."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn
    F, S, K, Hs, units = 16, 8, 3, 1, 30
    res = R.build_reservoir(R.SimulationParams(num_neurons=64, num_output_neurons=16, small_world_graph_k=16,
                                               mean_weight=2.0 / 8, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    rng = np.random.RandomState(48)
    pcm = (rng.standard_normal((N_STREAMS, units * 480)) * np.linspace(0.01, 0.5, units * 480)).astype(np.float32)

    def bank():
        return pipeline.AudioStreamBank(frontend.AdaptiveStream(_make_inner("gammatone", F), 100), net, S, K, Hs, ALL_KEYS,
                                        resampler=frontend.ResampleStream(48000, N_STREAMS))

    rows, counts = bank().push(pcm)
    assert counts.min() >= 1 and rows.any()
    cut, got, pos = bank(), [[] for _ in range(N_STREAMS)], 0
    for u in (1, 7, 22):
        r, c = cut.push(pcm[:, pos * 480:(pos + u) * 480])
        pos += u
        for b in range(N_STREAMS):
            got[b].append(r[b, :c[b]].cpu().numpy())
    for b in range(N_STREAMS):
        assert np.concatenate(got[b]).tobytes() == rows[b, :counts[b]].cpu().numpy().tobytes(), f"stream {b}"


# ---- (g) level -----------------------------------------------------------------------------------------------------------------
def test_a_quiet_stream_is_silent_with_a_fixed_range_and_spikes_with_the_adaptive_one(torch_cuda, oracle_c):
    """A chirp plus a little noise through 8 gammatone filters, at full level and 42 dB lower.  With the range calibrated
    on the loud copy the quiet copy's normalised values stay below 0.48 (on the oracle) and its raster is empty; with the
    sliding range of one second it spikes.  (The two adaptive rasters are not compared: the 1e-9 inside the logarithm
    makes the quiet copy's dB values no exact shift of the loud one's.)"""
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import frontend
    n = 16000
    t = np.arange(n) / 16000.0
    rng = np.random.RandomState(2027)
    loud = (0.5 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 * t * t)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    audio = np.stack([loud, loud * np.float32(2.0 ** -7)])
    # the statements on the CPU first, with the oracle
    coefs = ref_numpy.gammatone_coefs(16000, 8, 50)
    db = [20 * np.log10(oracle_c.gammatone_spec(a, coefs, 400, HOP, 98) + 1e-9) for a in audio]
    hi = float(db[0].max())
    lo = max(float(db[0].min()), hi - 80.0)
    fixed = [oracle_c.encode_hysteresis((np.maximum(d, hi - 80) - lo) / (hi - lo + 1e-8), THR4, GAP) for d in db]
    adaptive = [oracle_c.encode_hysteresis(A.adaptive(d, 100)[0], THR4, GAP) for d in db]
    assert fixed[0].sum() > 100 and fixed[1].sum() == 0 and adaptive[0].sum() > 100 and adaptive[1].sum() > 100
    assert ((np.maximum(db[1], hi - 80) - lo) / (hi - lo + 1e-8)).max() < 0.5
    # the device
    gs = frontend.GammatoneStream(8, 2, (lo, hi))
    raster, cols = gs.push(audio)
    assert cols.tolist() == [98, 98]
    raster = raster.cpu().numpy()
    assert raster[0].sum() > 100 and not raster[1].any(), "fixed range: the quiet stream is silent"
    ads = frontend.AdaptiveStream(frontend.GammatoneStream(8, 2, (lo, hi)), 100)
    raster, cols, db_dev = ads.push(audio, want_db=True)
    assert cols.tolist() == [98, 98]
    raster, db_dev = raster.cpu().numpy(), db_dev.cpu().numpy()
    assert raster[0].sum() > 100 and raster[1].sum() > 100, "adaptive range: both streams spike"
    for b in range(2):
        want = oracle_c.encode_hysteresis(A.adaptive(db_dev[b][:, :98], 100)[0], THR4, GAP)
        np.testing.assert_array_equal(raster[b][:, :98 * 4], want)
