"""Masks on ragged launches (SPEC.md 1.16, include/lsm_hip_ragged_augment.h; `SpikeFrontEnd.encode_ragged(mask=...)`).

Clip b of a masked ragged batch must be, byte for byte, what the masked UNRAGGED entry point gives for the clip alone on a
front end built for its T_b bins, under the first F and T_b bits of its mask rows -- and what the restatement gives
(tests/ragged_augment_restatement.py: tests/mask_restatement.py at the clip's own shape, over the oracle).  The unragged entry
points refuse a spectrogram of one column, which is what a gammatone clip of 3 bins has, so for that clip the restatement alone
is the reference (as in SPEC.md 1.14's tests).

The launch's stride is 40 time bins -- two mask words -- and the clips have 0, 3, 5, 31, 32, 33 and 40 bins.  The masks: a
frequency band on three clips; a time span over bins 30-34, which crosses the word boundary and the ends of the 31-, 32- and
33-bin clips; bin 1 of the 3-bin clip; the 5-bin clip has only bits behind its end, and EVERY clip's words have every bit from
T_b (and from F) on set: those are ignored.  Audio holds NaN behind every clip, dB input NaN behind a clip's columns, and the
outputs are pre-filled."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402
import ragged_augment_restatement as RA  # noqa: E402

pytestmark = pytest.mark.gpu

TB = 40
BINS = [0, 3, 5, 31, 32, 33, 40]
THR4 = [0.70, 0.80, 0.90, 0.95]
THR5 = [0.5, 0.6, 0.7, 0.8, 0.9]
GAP = 0.1
HOP = 160
_CACHE = {}


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
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _h(a):
    return C.c_void_p(a.ctypes.data)


def _dev_words(torch, words):
    return None if words is None else torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def masks(F):
    """-> (fm bool (7, F), tm bool (7, 40) -- what the definition reads --, freq words, time words -- what is launched)."""
    fm, tm = np.zeros((len(BINS), F), dtype=bool), np.zeros((len(BINS), TB), dtype=bool)
    band = slice(1, 3) if F <= 5 else slice(min(30, F - 3), min(34, F))         # F = 33: rows 30-32, across the word edge
    for b in (1, 3, 6):
        fm[b, band] = True
    tm[1, 1] = True
    for b in (3, 4, 5, 6):
        tm[b, 30:35] = True
    tm[0, 2:9] = True                                               # the empty clip: bits that no bin has
    wide_f = np.zeros((len(BINS), 32 * ((F + 31) // 32)), dtype=bool)
    wide_f[:, :F], wide_f[:, F:] = fm, True
    wide_t = np.zeros((len(BINS), 64), dtype=bool)
    for b, T in enumerate(BINS):
        wide_t[b, :T], wide_t[b, T:] = tm[b, :T], True
        tm[b, T:] = False
    freq, time = MR.words_of(wide_f), MR.words_of(wide_t)
    assert time.shape == (len(BINS), 2) and not tm[2].any() and time[2].any()
    return fm, tm, freq, time


def _plan_alone(fm, tm, b, T):
    from lsm_speech_classifier_amd import frontend
    return frontend.MaskPlan(MR.words_of(fm[b:b + 1]), MR.words_of(tm[b:b + 1, :T]))


# ---- 1. the split encoder ---------------------------------------------------------------------------------------------------
def _walk_db(seed, B, F, nc, dtype):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.standard_normal((B, F, nc)).cumsum(axis=2) * 4.0 - 30.0).astype(dtype))


def _encoder(torch, name, db, ncols, tb, cols, bins, floor, thr, red, freq=None, time=None):
    """One call of an lsm_spec_to_spikes_* export through the C ABI -> (raster, norm_out) from pre-filled buffers."""
    lib = _lib_()
    dt = db.dtype.type
    on = np.array(sorted(thr, reverse=True), dtype=dt)
    off = np.array([dt(t - GAP) for t in sorted(thr, reverse=True)], dtype=dt)
    B, F = db.shape[:2]
    d = torch.from_numpy(np.ascontiguousarray(db)).cuda()
    raster = torch.full((B, F * red, tb * len(thr)), 0xFF, dtype=torch.uint8, device="cuda")
    norm = torch.full((B, F, tb), -7.0, dtype=d.dtype, device="cuda")
    args = [_p(d), B, F, ncols, tb]
    if "ragged" in name:
        c, t = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (cols, bins))
        args += [_p(c), _p(t)]
    args += [floor, _h(on), _h(off), len(on), red, _p(raster), _p(norm)]
    if "masked" in name:
        fw, tw = _dev_words(torch, freq), _dev_words(torch, time)
        args += [_p(fw), _p(tw)]
    rc = getattr(lib, name)(*args, None)
    assert rc == 0, lib.lsm_last_error().decode()
    torch.cuda.synchronize()
    return raster.cpu().numpy(), norm.cpu().numpy()


@pytest.mark.parametrize("thr", [THR4, THR5], ids=["4thr", "5thr"])
@pytest.mark.parametrize("F", [5, 33])
@pytest.mark.parametrize("dtype,floor,extra", [(np.float64, 1, -2), (np.float32, 0, 1)], ids=["f64-floor", "f32"])
def test_split_encoder_clips_equal_the_masked_clip_alone_and_the_restatement(torch_cuda, dtype, floor, extra, F, thr):
    """`lsm_spec_to_spikes_ragged_masked_*`: a clip of T bins has T - 2 columns (the gammatone shapes, f64 with the floor) or
    T + 1 (the mel shapes, f32)."""
    torch = torch_cuda
    suffix = "f64" if dtype == np.float64 else "f32"
    red, n_thr = 2, len(thr)
    ncols = TB + extra
    cols = [max(T + extra, 0) if T else 0 for T in BINS]
    db = _walk_db(F + n_thr, len(BINS), F, ncols, dtype)
    poisoned = db.copy()
    for b, c in enumerate(cols):
        poisoned[b][:, c:] = np.nan
    fm, tm, freq, time = masks(F)
    raster, norm = _encoder(torch, "lsm_spec_to_spikes_ragged_masked_" + suffix, poisoned, ncols, TB, cols, BINS, floor, thr, red,
                            freq, time)
    want_norm, want = RA.masked_ragged([db[b][:, :c] for b, c in enumerate(cols)], BINS, TB, bool(floor), thr, GAP, red, freq, time,
                                       dtype)
    assert raster.tobytes() == want.tobytes(), "rasters against the restatement"
    assert norm.tobytes() == want_norm.tobytes(), "norm_out (S') against the restatement"
    plain, plain_norm = _encoder(torch, "lsm_spec_to_spikes_ragged_" + suffix, poisoned, ncols, TB, cols, BINS, floor, thr, red)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    changed = 0
    for b, (c, T) in enumerate(zip(cols, BINS)):
        assert not raster[b][:, T * n_thr:].any() and not norm[b][:, T:].view(bits).any(), f"clip {b}: the rest of its rows"
        if T == 0:
            continue
        cells = fm[b][:, None] | tm[b][None, :T]
        assert not norm[b][:, :T][cells].view(bits).any() and np.array_equal(norm[b][:, :T][~cells], plain_norm[b][:, :T][~cells])
        changed += raster[b].tobytes() != plain[b].tobytes()
        if c >= 2:                                                  # the masked unragged entry point on the clip alone
            alone = _plan_alone(fm, tm, b, T)
            r1, n1 = _encoder(torch, "lsm_spec_to_spikes_masked_" + suffix, np.ascontiguousarray(db[b:b + 1, :, :c]), c, T, None,
                              None, floor, thr, red, alone.freq, alone.time)
            assert raster[b][:, :T * n_thr].tobytes() == r1[0].tobytes(), f"clip {b} ({c} columns, {T} bins): raster"
            assert norm[b][:, :T].tobytes() == n1[0].tobytes(), f"clip {b}: norm_out"
    assert raster[2].tobytes() == plain[2].tobytes() and norm[2].tobytes() == plain_norm[2].tobytes()     # only ignored bits
    assert changed >= 4, "the masks changed hardly a raster"
    # clear masks and NULL masks: the unmasked ragged bytes; one kind at a time: the other pointer NULL
    for fw, tw in ((None, None), (np.zeros_like(freq), np.zeros_like(time)), (np.zeros_like(freq), None)):
        r0, n0 = _encoder(torch, "lsm_spec_to_spikes_ragged_masked_" + suffix, poisoned, ncols, TB, cols, BINS, floor, thr, red, fw, tw)
        assert r0.tobytes() == plain.tobytes() and n0.tobytes() == plain_norm.tobytes()
    only_t, _ = _encoder(torch, "lsm_spec_to_spikes_ragged_masked_" + suffix, poisoned, ncols, TB, cols, BINS, floor, thr, red, None, time)
    assert only_t.tobytes() == RA.masked_ragged([db[b][:, :c] for b, c in enumerate(cols)], BINS, TB, bool(floor), thr, GAP, red,
                                                None, time, dtype)[1].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_mask_releases_the_latch_on_a_ragged_row(torch_cuda, dtype):
    """SPEC.md 1.13's constructed row -- 0.75, 0.65, 0.65, ... beside a row 0, 1, threshold 0.7 with gap 0.1, bin 3 masked --
    as a clip of 33 bins in a launch of 40: on for bins 0-2, released by the masked bin and never set again, where the
    unmasked raster with step 3 zeroed is on again from bin 4.  Masking is not zeroing raster bytes."""
    torch = torch_cuda
    T = 33
    db = np.full((2, 2, TB), np.nan, dtype=dtype)
    db[:, 0, :T] = 0.65
    db[:, 0, 0] = 0.75
    db[:, 1, :T] = 0.0
    db[:, 1, 1] = 1.0
    tm = np.zeros((2, 64), dtype=bool)
    tm[0, 3] = True
    tm[:, T:] = True
    suffix = "f64" if dtype == np.float64 else "f32"
    raster, norm = _encoder(torch, "lsm_spec_to_spikes_ragged_masked_" + suffix, db, TB, TB, [T, T], [T, T], 0, [0.7], 1, None,
                            MR.words_of(tm))
    assert raster[0, 0].tolist() == [1, 1, 1] + [0] * (TB - 3) and raster[1, 0].tolist() == [1] * T + [0] * (TB - T)
    assert MR.zeroed_raster(raster[1][:, :T], 1, 1, None, tm[0, :T])[0].tolist() == [1, 1, 1, 0] + [1] * (T - 4)
    assert norm[0, 0, 3] == 0 and norm[1, 0, 3] != 0 and norm[0, 0, 4] == norm[1, 0, 4]


# ---- 2. the gammatone launches ------------------------------------------------------------------------------------------------
def _audio(n_clips, n_samples, seed=11):
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


def _poisoned(audio):
    x = audio.copy()
    for b, T in enumerate(BINS):
        x[b, HOP * T:] = np.nan
    return x


def _front_end(F, fb, T, thr):
    from lsm_speech_classifier_amd import frontend
    key = ("fe", F, fb, T, tuple(thr))
    if key not in _CACHE:
        _CACHE[key] = frontend.SpikeFrontEnd(F, fb, thresholds=thr, gap=GAP, time_bins=T, n_samples=HOP * T)
    return _CACHE[key]


def _encode(torch, fe, audio, plan, **kw):
    out = torch.full((len(BINS), fe.n_channels, fe.n_steps), 0xFF, dtype=torch.uint8, device="cuda")
    raster, steps = fe.encode_ragged(torch.from_numpy(_poisoned(audio)).cuda(), BINS, raster_out=out, mask=plan, **kw)
    torch.cuda.synchronize()
    assert raster.data_ptr() == out.data_ptr() and steps.cpu().tolist() == [T * len(fe.thresholds) for T in BINS]
    return raster.cpu().numpy()


def _restated_gammatone(oracle_c, F, thr, audio, freq, time):
    from lsm_speech_classifier_amd import frontend
    key = ("restated", F, tuple(thr))
    if key not in _CACHE:
        tab = frontend.gammatone_filter_table(16000, F, 50)
        dbs = [RA.gammatone_db(oracle_c, tab, audio[b], T) if T else None for b, T in enumerate(BINS)]
        _CACHE[key] = RA.masked_ragged(dbs, BINS, TB, True, thr, GAP, 1, freq, time)[1]
    return _CACHE[key]


LAYOUTS = {"lane-pair": ("4", False, 0), "two-chains": ("12", False, 2), "one-chain": ("12", True, 1)}


@pytest.mark.parametrize("thr", [THR4, THR5], ids=["4thr", "5thr"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gammatone_clips_equal_the_masked_clip_alone_and_the_restatement(torch_cuda, oracle_c, monkeypatch, layout, thr):
    """`lsm_gammatone_spikes_ragged_masked_f64` at 128 filters in its three layouts -- the hardware-queue count the library
    reads at every launch picks the lane pair, and the low-latency flag one chain per lane instead of two; it changes the
    layout, never a result -- and the split route, which must give the same bytes."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, n_thr = 128, len(thr)
    queues, low_latency, want_layout = LAYOUTS[layout]
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
    assert _lib_().lsm_gammatone_spikes_layout(len(BINS), F, 1 if low_latency else 0) == want_layout
    fe = _front_end(F, "gammatone", TB, thr)
    audio = _audio(len(BINS), HOP * TB)
    fm, tm, freq, time = masks(F)
    plan = frontend.MaskPlan(freq, time)
    got = _encode(torch, fe, audio, plan, fused=True, low_latency=low_latency)
    assert got.tobytes() == _restated_gammatone(oracle_c, F, thr, audio, freq, time).tobytes(), "against the restatement"
    split = _encode(torch, fe, audio, plan, fused=False)
    assert got.tobytes() == split.tobytes(), "the one-launch route and the split route differ"
    plain = _encode(torch, fe, audio, None, fused=True, low_latency=low_latency)
    for b, T in enumerate(BINS):
        assert not got[b][:, T * n_thr:].any(), f"clip {b}: bytes past its {T} bins"
        if T >= 4:
            alone = _front_end(F, "gammatone", T, thr).encode(np.ascontiguousarray(audio[b:b + 1, :HOP * T]), fused=True,
                                                              low_latency=low_latency, mask=_plan_alone(fm, tm, b, T))
            torch.cuda.synchronize()
            assert got[b][:, :T * n_thr].tobytes() == alone[0].cpu().numpy().tobytes(), f"clip {b} ({T} bins) against the clip alone"
        if T and b != 2:
            assert got[b].tobytes() != plain[b].tobytes(), f"clip {b}: the mask changed nothing"
    assert got[2].tobytes() == plain[2].tobytes() and not got[0].any()
    # clear and NULL masks: the unmasked ragged bytes
    clear = frontend.MaskPlan(np.zeros_like(freq), np.zeros_like(time))
    assert _encode(torch, fe, audio, clear, fused=True, low_latency=low_latency).tobytes() == plain.tobytes()
    assert _encode(torch, fe, audio, clear, fused=False).tobytes() == plain.tobytes()


def test_null_mask_pointers_make_the_ragged_launch(torch_cuda):
    """Through the C ABI: both pointers NULL give the unmasked entry point's bytes, one NULL masks the other kind only."""
    torch = torch_cuda
    lib = _lib_()
    from lsm_speech_classifier_amd import frontend
    F = 128
    fe = _front_end(F, "gammatone", TB, THR4)
    x = torch.from_numpy(_poisoned(_audio(len(BINS), HOP * TB))).cuda()
    fm, tm, freq, time = masks(F)
    on, off = frontend.threshold_tables(THR4, GAP, np.float64)
    bins = torch.tensor(BINS, dtype=torch.int32, device="cuda")
    ws = fe.new_workspace(len(BINS))

    def run(name, *mask_words):
        raster = torch.full((len(BINS), F, TB * 4), 0xFF, dtype=torch.uint8, device="cuda")
        words = [_dev_words(torch, w) for w in mask_words]
        rc = getattr(lib, name)(_p(x), len(BINS), HOP * TB, _p(fe.coefs), F, fe.nwin, fe.hop, fe.ncols, TB, _p(bins), _h(on), _h(off),
                                4, 1, _p(raster), None, _p(ws), ws.numel() * 8, fe.coef_flags, 0, *[_p(w) for w in words], None)
        assert rc == 0, lib.lsm_last_error().decode()
        torch.cuda.synchronize()
        return raster.cpu().numpy()

    plain = run("lsm_gammatone_spikes_ragged_f64")
    assert run("lsm_gammatone_spikes_ragged_masked_f64", None, None).tobytes() == plain.tobytes()
    both = run("lsm_gammatone_spikes_ragged_masked_f64", freq, time)
    only_f, only_t = run("lsm_gammatone_spikes_ragged_masked_f64", freq, None), run("lsm_gammatone_spikes_ragged_masked_f64", None, time)
    assert both.tobytes() == _encode(torch, fe, _audio(len(BINS), HOP * TB), frontend.MaskPlan(freq, time), fused=True).tobytes()
    assert only_f.tobytes() == _encode(torch, fe, _audio(len(BINS), HOP * TB), frontend.MaskPlan(freq, np.zeros_like(time)), fused=True).tobytes()
    assert only_t.tobytes() == _encode(torch, fe, _audio(len(BINS), HOP * TB), frontend.MaskPlan(np.zeros_like(freq), time), fused=True).tobytes()
    assert len({plain.tobytes(), both.tobytes(), only_f.tobytes(), only_t.tobytes()}) == 4


# ---- 3. mel ---------------------------------------------------------------------------------------------------------------------
def test_mel_clips_equal_their_masked_clip_alone_runs(torch_cuda):
    """The mel branch's ragged route is the split route: `encode_ragged(mask=...)` against the mel front end's own masked
    unragged run on the clip alone, on the GPU (as SPEC.md 1.14's mel tests compare)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F = 13
    fe = _front_end(F, "mel", TB, THR4)
    audio = _audio(len(BINS), HOP * TB, seed=23)
    fm, tm, freq, time = masks(F)
    got = _encode(torch, fe, audio, frontend.MaskPlan(freq, time))
    plain = _encode(torch, fe, audio, None)
    for b, T in enumerate(BINS):
        assert not got[b][:, T * 4:].any()
        if T == 0:
            continue
        alone = _front_end(F, "mel", T, THR4).encode(np.ascontiguousarray(audio[b:b + 1, :HOP * T]), mask=_plan_alone(fm, tm, b, T))
        torch.cuda.synchronize()
        assert got[b][:, :T * 4].tobytes() == alone[0].cpu().numpy().tobytes(), f"clip {b} ({T} bins) against the clip alone"
    assert got[2].tobytes() == plain[2].tobytes() and sum(got[b].tobytes() != plain[b].tobytes() for b in range(len(BINS))) >= 3
