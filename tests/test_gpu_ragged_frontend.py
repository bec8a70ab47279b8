"""Clips of different lengths in one front-end launch (SPEC.md 1.14, include/lsm_hip_ragged.h, `SpikeFrontEnd.encode_ragged`).

Clip b of a ragged batch, T_b time bins long, must be byte for byte the raster of the front end built for that length
(`SpikeFrontEnd(..., n_samples=160 * T_b, time_bins=T_b)`) on the clip alone.  Every comparison is byte equality.  In every
test the audio rows hold NaN from a clip's end on, dB input holds NaN past a clip's columns, and the outputs are pre-filled
(0xFF raster bytes, -7 in norm_out): a kernel that reads past a clip's counts, or leaves the rest of a row unwritten, fails.
The device step counts must equal ``bins * n_thr`` throughout.

References.  Gammatone: the plain-C oracle (oracle/lsm_oracle.c) on the clip alone, and the same package's unragged launch on
the clip alone wherever that launch exists -- the unragged entry points refuse a spectrogram of ONE column, which is what a
clip of 3 bins has (400-sample windows, hop 160: T - 2 columns), so for T_b = 3 the oracle is the reference.  The encoder on
its own: `lsm_spec_to_spikes_*` on each clip alone (two columns or more) and the restated definition
(tests/encoder_restatement.py over the oracle's SciPy-exact resize) for every clip.  Mel: the mel front end's own unragged
run on the clip alone, on the GPU (NumPy's einsum projection differs from itself between the two shapes)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_restatement as ER  # noqa: E402

pytestmark = pytest.mark.gpu

THR = [0.70, 0.80, 0.90, 0.95]
THR5 = [0.5, 0.6, 0.7, 0.8, 0.9]            # more than 4 thresholds: the fused kernel's 8-bit fields
THR3 = [0.7, 0.8, 0.9]                      # 3 thresholds x 7 bins: 21-byte rows, the byte path of the row stores
GAP = 0.1
HOP = 160
BINS12 = [12, 3, 7, 0, 11, 4]
_LAYOUTS_OWN, _LAYOUTS_SCARCE = set(), set()        # fused layouts exercised with the process's queues / with 4 asked for


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _lib_():
    from lsm_speech_classifier_amd import _lib
    return _lib.load()


def _p(t):
    return C.c_void_p(t if isinstance(t, int) else (t.data_ptr() if t is not None else 0))


def _h(a):
    return C.c_void_p(a.ctypes.data)


def _queues():
    v = os.environ.get("GPU_MAX_HW_QUEUES")
    return int(v) if v and int(v) > 0 else 4


# ---- inputs and references (built once, shared, never written) ---------------------------------------------------------
_CACHE = {}


def _audio(seed, n_clips, n_samples):
    """Seeded clips: three sliding tones and noise, so that every stretch of a clip has its own level and spectrum."""
    key = ("audio", seed, n_clips, n_samples)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        t = np.arange(n_samples) / 16000.0
        x = 0.02 * rng.standard_normal((n_clips, n_samples))
        for b in range(n_clips):
            for _ in range(3):
                f0, f1, a = rng.uniform(100, 6000), rng.uniform(100, 6000), rng.uniform(0.05, 0.5)
                x[b] += a * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / t[-1])) * (0.3 + np.abs(np.sin(2 * np.pi * rng.uniform(2, 20) * t)))
        a = np.ascontiguousarray(x.astype(np.float32))
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def _poisoned(audio, bins):
    """A copy of the rows with NaN from each clip's end (160 * T_b) on."""
    x = audio.copy()
    for b, t in enumerate(bins):
        x[b, HOP * max(0, min(int(t), x.shape[1] // HOP)):] = np.nan
    return x


def _front_end(F, fb, T, red=1, thr=THR):
    from lsm_speech_classifier_amd import frontend
    key = ("fe", F, fb, T, red, tuple(thr))
    if key not in _CACHE:
        _CACHE[key] = frontend.SpikeFrontEnd(F, fb, redundancy=red, thresholds=thr, gap=GAP, time_bins=T, n_samples=HOP * T)
    return _CACHE[key]


def _oracle_clip(oracle_c, F, clip, T, red, thr):
    """The oracle's raster of one gammatone clip of T bins, alone: gtgram with (400, 160, T - 2), floor, normalise, zoom to T."""
    from lsm_speech_classifier_amd import frontend
    key = ("oracle", F, clip.tobytes(), T, red, tuple(thr))
    if key not in _CACHE:
        coefs = frontend.gammatone_filter_table(16000, F, 50)
        with np.errstate(all="ignore"):
            r = oracle_c.encode_hysteresis(oracle_c.normalise_resize(oracle_c.gammatone_db(
                oracle_c.gammatone_spec(clip, coefs, 400, HOP, T - 2)), T), thr, GAP)
        _CACHE[key] = np.repeat(r, red, axis=0)
    return _CACHE[key]


def _alone(torch, F, fb, clip, T, red, thr):
    """The unragged front end of this length on the clip alone (GPU), or None where its launch does not exist (one column)."""
    if fb == "gammatone" and T - 2 < 2:
        return None
    fe = _front_end(F, fb, T, red, thr)
    out = fe.encode(clip[None].copy())
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def _check_rows(torch, oracle_c, fb, F, red, thr, audio, bins, got, steps, tb):
    n_thr = len(thr)
    got = got.cpu().numpy()
    assert got.shape == (len(bins), F * red, tb * n_thr)
    assert steps.dtype == torch.int32 and steps.cpu().tolist() == [int(t) * n_thr for t in bins]
    some = 0
    for b, T in enumerate(bins):
        own, rest = got[b][:, :T * n_thr], got[b][:, T * n_thr:]
        assert not rest.any(), f"clip {b}: bytes past its {T} bins are not zero"
        if T == 0:
            continue
        clip = np.ascontiguousarray(audio[b, :HOP * T])
        alone = _alone(torch, F, fb, clip, T, red, thr)
        if alone is not None:
            assert np.array_equal(own, alone), f"clip {b} ({T} bins) differs from the front end of that length on it alone"
        if fb == "gammatone":
            assert np.array_equal(own, _oracle_clip(oracle_c, F, clip, T, red, thr)), f"clip {b} ({T} bins) differs from the oracle"
        some += int(own.any())
    assert some >= sum(1 for t in bins if t) - 1, "the clips' rasters are (nearly) all empty: the comparison shows nothing"


def _encode(torch, fe, audio, bins, **kw):
    """encode_ragged on NaN-tailed rows into a 0xFF-filled raster."""
    out = torch.full((len(bins), fe.n_channels, fe.n_steps), 0xFF, dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(_poisoned(audio, bins)).cuda()
    raster, steps = fe.encode_ragged(x, bins, raster_out=out, **kw)
    torch.cuda.synchronize()
    assert raster.data_ptr() == out.data_ptr()
    return raster, steps


# ---- 1. the fused gammatone launch -----------------------------------------------------------------------------------------
FUSED_CASES = {                 # F, redundancy, thresholds, time_bins, bins
    "lane-pair-F8": (8, 1, THR, 12, BINS12),
    "partly-live-group-F70-r2": (70, 2, THR, 12, BINS12),
    "F260": (260, 1, THR, 6, [6, 3, 5]),
    "five-thresholds": (33, 1, THR5, 12, BINS12),
    "rows-of-21-bytes": (40, 1, THR3, 7, [7, 3, 5, 0, 6]),
}


@pytest.mark.parametrize("queues", ["own", "4"])
@pytest.mark.parametrize("low_latency", [False, True], ids=["flags0", "flags1"])
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_gammatone_clips_equal_their_clip_alone_runs(torch_cuda, oracle_c, monkeypatch, case, low_latency, queues):
    """`lsm_gammatone_spikes_ragged_f64`: every clip against the unragged launch of its length and against the oracle, in
    the layout the process's hardware queues select and in the one that 4 queues select (the lane pair up to 256 filters:
    the variable is read at every launch and changes the layout, never a result)."""
    torch = torch_cuda
    F, red, thr, tb, bins = FUSED_CASES[case]
    if queues == "4":
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    layout = _lib_().lsm_gammatone_spikes_layout(len(bins), F, 1 if low_latency else 0)
    assert layout in (0, 1, 2)
    if queues == "4":
        assert layout == (0 if F <= 256 else (1 if low_latency else 2))
    fe = _front_end(F, "gammatone", tb, red, thr)
    audio = _audio(11, len(bins), HOP * tb)
    raster, steps = _encode(torch, fe, audio, bins, fused=True, low_latency=low_latency)
    (_LAYOUTS_SCARCE if queues == "4" else _LAYOUTS_OWN).add(layout)
    _check_rows(torch, oracle_c, "gammatone", F, red, thr, audio, bins, raster, steps, tb)
    if (tb * len(thr)) & 3:
        assert case == "rows-of-21-bytes"


def test_fused_layouts_exercised(torch_cuda):
    """Runs after the cases above (file order): with the process's own queue count the fused launches took every layout that
    count offers -- the lane pair, one chain and two chains with at most 4 hardware queues, the two chain layouts with more
    -- and, asked for 4 queues, the lane pair and the chain layouts of 260 filters."""
    assert _LAYOUTS_OWN == ({0, 1, 2} if _queues() <= 4 else {1, 2}), (_queues(), _LAYOUTS_OWN)
    assert _LAYOUTS_SCARCE == {0, 1, 2}, _LAYOUTS_SCARCE


# ---- 2. the split gammatone route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lane-pair-F8", "partly-live-group-F70-r2", "rows-of-21-bytes"])
def test_split_route_gives_the_fused_bytes_and_the_clip_alone_norm(torch_cuda, oracle_c, case):
    torch = torch_cuda
    F, red, thr, tb, bins = FUSED_CASES[case]
    fe = _front_end(F, "gammatone", tb, red, thr)
    audio = _audio(11, len(bins), HOP * tb)
    fused, steps_f = _encode(torch, fe, audio, bins, fused=True)
    split, steps_s = _encode(torch, fe, audio, bins, fused=False)
    assert torch.equal(fused, split) and torch.equal(steps_f, steps_s)
    _check_rows(torch, oracle_c, "gammatone", F, red, thr, audio, bins, split, steps_s, tb)
    # norm_out of the ragged encoder on the padded rows' dB values: the clip-alone norm_out, zeros past T_b
    x = torch.from_numpy(_poisoned(audio, bins)).cuda()
    db, _ = fe.spectrogram_db(x)
    t = torch.tensor(bins, dtype=torch.int32, device="cuda")
    cols = torch.where(t > 0, t - 2, torch.zeros_like(t)).contiguous()
    raster, norm = fe.spikes_from_db_ragged(db, cols, t, want_norm=True)
    torch.cuda.synchronize()
    assert torch.equal(raster, fused)
    norm, db_h = norm.cpu().numpy(), db.cpu().numpy()
    on, off = ER.tables(thr, GAP, np.float64)
    for b, T in enumerate(bins):
        assert not norm[b][:, T:].any() and not np.signbit(norm[b][:, T:]).any()
        if T == 0:
            continue
        want, _ = ER.expected(oracle_c, np.ascontiguousarray(db_h[b][:, :T - 2]), T, on, off)      # the definition
        assert np.array_equal(norm[b][:, :T].view(np.uint64), want.view(np.uint64)), f"clip {b}: norm_out"
        if T - 2 >= 2:
            fe_t = _front_end(F, "gammatone", T, red, thr)
            db_t, _ = fe_t.spectrogram_db(np.ascontiguousarray(audio[b:b + 1, :HOP * T]))
            assert torch.equal(db_t[0], db[b][:, :T - 2]), f"clip {b}: the padded row's columns are not the clip's own"
            _, norm_t = fe_t.spikes_from_db(db_t, want_norm=True)
            assert np.array_equal(norm[b][:, :T].view(np.uint64), norm_t[0].cpu().numpy().view(np.uint64)), f"clip {b}"


# ---- 3. the ragged encoder on its own --------------------------------------------------------------------------------------
ENC_STRIDE = 30
ENC_PAIRS = [(28, 27), (5, 5), (1, 3), (10, 12), (0, 0), (10, 12), (10, 12), (30, 30), (2, 30)]     # (cols, bins) per clip
ENC_FLAT, ENC_NAN = 5, 6


def _encoder_db(dtype):
    key = ("encdb", np.dtype(dtype).name)
    if key not in _CACHE:
        db = ER.walk_db(5, len(ENC_PAIRS), 7, ENC_STRIDE, dtype).copy()
        db[ENC_FLAT] = dtype(-31.25)
        db[ENC_NAN, 3, 4] = np.nan
        db.setflags(write=False)
        _CACHE[key] = db
    return _CACHE[key]


def _call_encoder(torch, name, dt, db, ncols, tb, cols, bins, floor, on, off, red, want_norm=True, stream=None):
    lib = _lib_()
    B, F = db.shape[0], db.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(db)).cuda()
    raster = torch.full((B, F * red, tb * len(on)), 0xFF, dtype=torch.uint8, device="cuda")
    norm = torch.full((B, F, tb), -7.0, dtype=d.dtype, device="cuda") if want_norm else None
    head = [_p(d), B, F, ncols, tb]
    tail = [floor, _h(on), _h(off), len(on), red, _p(raster), _p(norm), stream]
    rc = getattr(lib, name)(*(head + ([_p(cols), _p(bins)] if "ragged" in name else []) + tail))
    torch.cuda.synchronize()
    return rc, raster.cpu().numpy(), (norm.cpu().numpy() if want_norm else None)


@pytest.mark.parametrize("dtype,floor", [(np.float64, 1), (np.float32, 0)], ids=["f64-floor", "f32"])
def test_ragged_encoder_on_its_own(torch_cuda, oracle_c, dtype, floor):
    """`lsm_spec_to_spikes_ragged_*` at strides 30 x 30: (28, 27) is the smallest mel shape (T + 1 columns) whose last bin
    overshoots and must be +0.0 -- no gammatone shape below 400 bins does, so the fused tests cannot reach that rule --, (5, 5)
    takes no zoom, (1, 3) is the shortest clip, (0, 0) is empty, one clip is flat, one holds a NaN, one is the full stride."""
    torch = torch_cuda
    suffix = "f64" if dtype == np.float64 else "f32"
    red = 2
    assert ER.overshoots(28, 27) and not any(ER.overshoots(c, t) for c, t in ENC_PAIRS[1:] if t)
    assert not any(ER.overshoots(T - 2, T) for T in range(4, 400))
    db = _encoder_db(dtype)
    poisoned = db.copy()
    for b, (c, _) in enumerate(ENC_PAIRS):
        poisoned[b][:, c:] = np.nan
    on, off = ER.tables(THR, GAP, dtype)
    cols = torch.tensor([c for c, _ in ENC_PAIRS], dtype=torch.int32, device="cuda")
    bins = torch.tensor([t for _, t in ENC_PAIRS], dtype=torch.int32, device="cuda")
    rc, raster, norm = _call_encoder(torch, "lsm_spec_to_spikes_ragged_" + suffix, dtype, poisoned, ENC_STRIDE, ENC_STRIDE, cols,
                                     bins, floor, on, off, red)
    assert rc == 0, _lib_().lsm_last_error().decode()
    bits = np.uint64 if dtype == np.float64 else np.uint32
    for b, (c, T) in enumerate(ENC_PAIRS):
        assert not raster[b][:, T * len(on):].any() and not norm[b][:, T:].any(), f"clip {b}: the rest of its rows"
        assert not np.signbit(norm[b][:, T:]).any()
        if T == 0:
            continue
        clip = np.ascontiguousarray(db[b][:, :c])
        want_norm, want_raster = ER.expected(oracle_c, clip, T, on, off, apply_floor=bool(floor), redundancy=red)
        if b == ENC_NAN:                                            # (a NaN's payload is nobody's contract)
            assert np.isnan(want_norm).all() and np.isnan(norm[b][:, :T]).all()
        else:
            assert np.array_equal(norm[b][:, :T].view(bits), want_norm.view(bits)), f"clip {b} {c, T}: norm_out against the definition"
        assert np.array_equal(raster[b][:, :T * len(on)], want_raster), f"clip {b} {c, T}: raster against the definition"
        if c >= 2:                                                  # the unragged entry point on the clip alone
            rc1, r1, n1 = _call_encoder(torch, "lsm_spec_to_spikes_" + suffix, dtype, clip[None], c, T, None, None, floor, on, off, red)
            assert rc1 == 0
            assert np.array_equal(raster[b][:, :T * len(on)], r1[0]), f"clip {b} {c, T}: raster against the clip alone"
            assert np.array_equal(norm[b][:, :T], n1[0], equal_nan=True), f"clip {b} {c, T}: norm_out against the clip alone"
    assert (norm[0][:, 26] == 0).all() and not np.signbit(norm[0][:, 26]).any() and norm[0][:, 25].any()    # the zero rule
    assert not raster[ENC_FLAT].any() and not norm[ENC_FLAT].any()                                             # flat: zeros
    assert not raster[ENC_NAN].any() and np.isnan(norm[ENC_NAN][:, :12]).all()                                 # NaN clip
    assert raster[3].any() and raster[7].any() and raster[0].any()


# ---- 4. mel ----------------------------------------------------------------------------------------------------------------
def test_mel_clips_equal_their_clip_alone_runs(torch_cuda, oracle_c):
    torch = torch_cuda
    F, tb, bins = 13, 30, [30, 27, 3, 0, 16]
    fe = _front_end(F, "mel", tb)
    audio = _audio(23, len(bins), HOP * tb)
    raster, steps = _encode(torch, fe, audio, bins)
    _check_rows(torch, oracle_c, "mel", F, 1, THR, audio, bins, raster, steps, tb)
    with pytest.raises(ValueError, match="no one-launch ragged kernel"):
        fe.encode_ragged(audio, bins, fused=True)


def test_power_to_db_ragged_takes_its_reference_over_the_clips_frames(torch_cuda):
    """`lsm_power_to_db_ragged_f32` against `lsm_power_to_db_f32` on each clip's frames alone: the loudest value of the padded
    rows lies past the clip's frames and must not become its reference; columns past the frames are written as 0."""
    torch = torch_cuda
    lib = _lib_()
    rng = np.random.default_rng(2)
    B, M, NF = 6, 5, 31
    frames = [31, 28, 4, 0, 17, 1]
    power = (10.0 ** rng.uniform(-12, 1, (B, M, NF))).astype(np.float32)
    power[4, 2, 3] = np.nan
    for b, n in enumerate(frames):
        power[b][:, n:] = 1e6
    power[2][:, 4:] = np.nan
    p = torch.from_numpy(power).cuda()
    out = torch.full((B, M, NF), -7.0, dtype=torch.float32, device="cuda")
    cf = torch.tensor(frames, dtype=torch.int32, device="cuda")
    rc = lib.lsm_power_to_db_ragged_f32(_p(p), B, M, NF, _p(cf), C.c_float(1e-10), C.c_float(80.0), _p(out), None)
    assert rc == 0, lib.lsm_last_error().decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b, n in enumerate(frames):
        assert not got[b][:, n:].any()
        if n == 0:
            continue
        alone = torch.from_numpy(np.ascontiguousarray(power[b][:, :n])).cuda()
        ref = torch.empty_like(alone)
        assert lib.lsm_power_to_db_f32(_p(alone), 1, M * n, C.c_float(1e-10), C.c_float(80.0), _p(ref), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(got[b][:, :n], ref.cpu().numpy().reshape(M, n), equal_nan=True), f"clip {b}"
    assert np.isnan(got[4][:, :17]).all() and got[0].max() == 0.0 and got[0].min() >= -80.0


# ---- 5. clamping -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb,fused", [("gammatone", True), ("gammatone", False), ("mel", False)])
def test_device_counts_are_clamped(torch_cuda, fb, fused):
    """Counts -1, 1, 2 and time_bins + 5 in a device tensor (never read on the host) behave as 0, 0, 0 and time_bins."""
    torch = torch_cuda
    tb = 12
    fe = _front_end(8, fb, tb)
    audio = _audio(31, 5, HOP * tb)
    wild, tame = [-1, 1, 2, tb + 5, 7], [0, 0, 0, tb, 7]
    want, want_steps = _encode(torch, fe, audio, tame, fused=fused)
    out = torch.full_like(want, 0xFF)
    x = torch.from_numpy(_poisoned(audio, tame)).cuda()
    got, steps = fe.encode_ragged(x, torch.tensor(wild, dtype=torch.int32, device="cuda"), fused=fused, raster_out=out)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and steps.cpu().tolist() == want_steps.cpu().tolist() == [0, 0, 0, tb * 4, 28]
    assert not got[:3].any() and got[3].any() and got[4].any()
    with pytest.raises(ValueError, match="of clips"):                 # the same values from the host are refused
        fe.encode_ragged(x, wild, fused=fused)


def test_encoder_counts_are_clamped(torch_cuda):
    """The split encoder's own clamp: columns above the stride, negative columns, a clip without a column."""
    torch = torch_cuda
    db = _encoder_db(np.float64)[:5]
    on, off = ER.tables(THR, GAP, np.float64)
    def run(cols, bins):
        c = torch.tensor(cols, dtype=torch.int32, device="cuda")
        t = torch.tensor(bins, dtype=torch.int32, device="cuda")
        rc, r, n = _call_encoder(torch, "lsm_spec_to_spikes_ragged_f64", np.float64, db, ENC_STRIDE, ENC_STRIDE, c, t, 1, on, off, 1)
        assert rc == 0
        return r, n
    want_r, want_n = run([30, 0, 0, 10, 0], [30, 0, 0, 12, 0])
    got_r, got_n = run([2 ** 31 - 1, -5, 0, 10, 10], [35, 12, 12, 12, 2])
    assert np.array_equal(got_r, want_r) and np.array_equal(got_n.view(np.uint64), want_n.view(np.uint64))
    assert want_r[0].any() and want_r[3].any() and not want_r[[1, 2, 4]].any()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------
UTTERANCE_SAMPLES = [480, 1920, 700, 1000, 1601, 481, 1300]
KEYS = ["spike_counts", "spike_variances", "last_spike_times", "mean_isi"]


@pytest.mark.parametrize("fb", ["gammatone", "mel"])
def test_features_from_utterances_equal_the_clip_alone_pipeline(torch_cuda, oracle_c, monkeypatch, fb):
    """Seven utterances of 480 .. 1920 samples through `pipeline.features_from_utterances`, in one batch, in batches of three
    and with the reservoir forced into chunks: row r is, bit for bit, the front end of utterance r's length on it alone
    followed by `run_batch` on that raster alone (the smallest reservoir of tests/test_gpu_ragged.py)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import pipeline, reservoir as R, snn
    n, k, n_out, c = 256, 50, 100, 40
    net = snn.SNN(None, reservoir=R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out,
                                                                       small_world_graph_k=k, mean_weight=2.0 / (k // 2),
                                                                       refractory_period=2), c))
    F, red, tb = 20, 2, 12
    fe = _front_end(F, fb, tb, red)
    utts = [np.ascontiguousarray(_audio(41, 7, 1920)[r, :m]) + np.float32(0.0) for r, m in enumerate(UTTERANCE_SAMPLES)]
    want = []
    for u in utts:
        T = -(-len(u) // HOP)
        clip = np.zeros(HOP * T, np.float32)
        clip[:len(u)] = u
        raster = _alone(torch, F, fb, clip, T, red, THR)
        if raster is None:                                          # 3 bins of gammatone: one column, the oracle's raster
            raster = _oracle_clip(oracle_c, F, clip, T, red, THR)
        f, _, _ = net.run_batch(np.ascontiguousarray(raster[None]), KEYS)
        torch.cuda.synchronize()
        want.append(f[0].cpu().numpy())
    want = np.stack(want)
    # the reference must tell the utterances apart (the shortest ones may leave this small reservoir silent: rows of zeros)
    live = want[want.any(axis=1)]
    assert len(live) >= 4 and len({w.tobytes() for w in live}) == len(live)
    got = pipeline.features_from_utterances(utts, fe, net, KEYS)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    got3 = pipeline.features_from_utterances(utts, fe, net, KEYS, batch=3)
    assert torch.equal(got3, got)
    monkeypatch.setattr(net, "max_steps", lambda n_clips, waves_per_clip=0: 20)      # 48 steps: three launches per batch
    chunked = pipeline.features_from_utterances(utts, fe, net, KEYS)
    assert torch.equal(chunked, got)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def _refused(torch, rc, code, raster, word):
    torch.cuda.synchronize()
    msg = _lib_().lsm_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert bool((raster == 0xFF).all()), "a refused call launched something"


def test_refusals_return_their_code_with_a_message_and_launch_nothing(torch_cuda):
    torch = torch_cuda
    lib = _lib_()
    from lsm_speech_classifier_amd import frontend
    ARG, UNSUPPORTED = -1, -4
    B, F, tb = 2, 8, 12
    fe = _front_end(F, "gammatone", tb)
    on, off = ER.tables(THR, GAP, np.float64)
    audio = torch.from_numpy(_audio(11, B, HOP * tb)).cuda()
    bins = torch.tensor([12, 5, 0], dtype=torch.int32, device="cuda")           # (one spare entry: a misaligned view of 2)
    steps = torch.zeros(3, dtype=torch.int32, device="cuda")
    raster = torch.full((B, F, tb * 4), 0xFF, dtype=torch.uint8, device="cuda")
    ws_bytes = int(lib.lsm_gammatone_spikes_workspace(B, 1025, tb - 1))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")

    def fused(**kw):
        a = dict(audio=_p(audio), n_clips=B, n_samples=HOP * tb, coefs=_p(fe.coefs), n_filters=F, nwin=400, hop=HOP,
                 ncols=tb - 2, time_bins=tb, clip_bins=_p(bins), on=_h(on), off=_h(off), n_thr=4, red=1, raster=_p(raster),
                 steps=_p(steps), ws=_p(ws), ws_bytes=ws_bytes, coef_flags=fe.coef_flags, flags=0)
        a.update(kw)
        return lib.lsm_gammatone_spikes_ragged_f64(*a.values(), None)

    assert fused(raster=_p(torch.full_like(raster, 0xFF))) == 0                  # the call itself is sound
    # the twin's refusals, in the twin's order, before the ragged ones (the count array is NULL in each)
    _refused(torch, fused(flags=4, clip_bins=None), ARG, raster, "launch_flags")
    _refused(torch, fused(n_filters=1, clip_bins=None), ARG, raster, "n_filters >= 2")
    _refused(torch, fused(ncols=tb - 1, clip_bins=None), ARG, raster, "columns exceed the clip")
    _refused(torch, fused(n_thr=9, clip_bins=None), ARG, raster, "n_thr")
    _refused(torch, fused(ws_bytes=8, clip_bins=None), ARG, raster, "workspace")
    _refused(torch, fused(n_filters=1025, clip_bins=None), UNSUPPORTED, raster, "waves per clip")
    # then: NULL, alignment, time_bins < 3, rows shorter than hop * time_bins
    _refused(torch, fused(clip_bins=None), ARG, raster, "null per-clip count array")
    _refused(torch, fused(clip_bins=_p(bins.data_ptr() + 2)), ARG, raster, "4-byte aligned")
    _refused(torch, fused(steps=_p(steps.data_ptr() + 1)), ARG, raster, "clip_steps_out")
    _refused(torch, fused(time_bins=2, ncols=2, nwin=160, n_samples=480), ARG, raster, "at least 3 time bins")
    _refused(torch, fused(n_samples=HOP * tb - 1), ARG, raster, "hop * time_bins")
    _refused(torch, fused(clip_bins=_p(bins.data_ptr() + 2), time_bins=2, ncols=2, nwin=160, n_samples=480), ARG, raster,
             "4-byte aligned")                                                   # alignment comes before the strides
    assert fused(steps=None, raster=_p(torch.full_like(raster, 0xFF))) == 0      # clip_steps_out may be NULL

    for suffix, dt in (("f64", np.float64), ("f32", np.float32)):
        on_t, off_t = ER.tables(THR, GAP, dt)
        db = torch.from_numpy(_encoder_db(dt)[:B].copy()).cuda()
        cols = torch.tensor([10, 5, 0], dtype=torch.int32, device="cuda")
        r2 = torch.full((B, 7, ENC_STRIDE * 4), 0xFF, dtype=torch.uint8, device="cuda")
        fn = getattr(lib, "lsm_spec_to_spikes_ragged_" + suffix)

        def enc(**kw):
            a = dict(db=_p(db), n_clips=B, F=7, ncols=ENC_STRIDE, tb=ENC_STRIDE, cols=_p(cols), bins=_p(bins), floor=1,
                     on=_h(on_t), off=_h(off_t), n_thr=4, red=1, raster=_p(r2), norm=None)
            a.update(kw)
            return fn(*a.values(), None)

        assert enc(raster=_p(torch.full_like(r2, 0xFF))) == 0
        _refused(torch, enc(n_thr=9, cols=None), ARG, r2, "n_thr")               # the twin's first
        _refused(torch, enc(ncols=1, cols=None), ARG, r2, "bad shape")
        _refused(torch, enc(cols=None), ARG, r2, "null per-clip count array")
        _refused(torch, enc(bins=None), ARG, r2, "null per-clip count array")
        _refused(torch, enc(cols=_p(cols.data_ptr() + 2)), ARG, r2, "4-byte aligned")
        _refused(torch, enc(bins=_p(bins.data_ptr() + 1)), ARG, r2, "4-byte aligned")
        _refused(torch, enc(tb=2), ARG, r2, "at least 3 time bins")

    power = torch.ones((B, 5, 13), dtype=torch.float32, device="cuda")
    out = torch.full((B, 5, 13), -7.0, dtype=torch.float32, device="cuda")

    def p2db(**kw):
        a = dict(power=_p(power), n_clips=B, n_mels=5, n_frames=13, frames=_p(bins), amin=C.c_float(1e-10), top=C.c_float(80.0),
                 out=_p(out))
        a.update(kw)
        rc = lib.lsm_power_to_db_ragged_f32(*a.values(), None)
        torch.cuda.synchronize()
        return rc, lib.lsm_last_error().decode()

    for kw, word in ((dict(n_frames=0), "bad shape"), (dict(power=None), "null buffer"), (dict(frames=None), "null clip_frames"),
                     (dict(frames=_p(bins.data_ptr() + 2)), "4-byte aligned")):
        rc, msg = p2db(**kw)
        assert rc == ARG and word in msg and bool((out == -7.0).all()), (kw, rc, msg)
    assert p2db()[0] == 0

    # Python: a front end of another shape, host bins out of range, buffers of the wrong kind
    other = frontend.SpikeFrontEnd(F, "gammatone")                               # 16000 samples, 100 bins: ragged-capable
    assert frontend.ragged_refusal(other.n_samples, other.time_bins) is None
    odd = frontend.SpikeFrontEnd(F, "gammatone", n_samples=2000, time_bins=12)
    with pytest.raises(ValueError, match="n_samples = 1920"):
        odd.encode_ragged(np.zeros((1, 2000), np.float32), [5])
    with pytest.raises(ValueError, match="of clips"):
        fe.encode_ragged(audio, [13, 5])
    with pytest.raises(ValueError, match="raster_out"):
        fe.encode_ragged(audio, [12, 5], raster_out=torch.zeros((B, F, 47), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="workspace belongs to the fused launch"):
        fe.encode_ragged(audio, [12, 5], fused=False, workspace=ws)
