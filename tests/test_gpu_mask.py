"""Masks inside the spike encoders on the device (SPEC.md 1.13, include/lsm_hip_mask.h): the split entry points, the fused
gammatone launch in every layout, the mel one-launch route and `pipeline.HotPath` against the NumPy restatement of the
definition (tests/mask_restatement.py) and against each other, byte for byte; clear masks against the unmasked twins; the
refusals.  Two conditions keep the comparisons from being vacuous (`test_fused_gammatone_...`): every masked clip's raster
differs from its unmasked raster, and in at least one clip it also differs from the unmasked raster with the masked rows and
steps zeroed -- an encoder that only zeroed raster bytes would not pass."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu

THR = [0.70, 0.80, 0.90, 0.95]
THR8 = [0.3, 0.6, 0.65, 0.7, 0.8, 0.9, 0.95, 0.99]
GAP = 0.1
TB = 100


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


def _words_dev(torch, words):
    """uint32 host words -> the same bits in an int32 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def hand_masks(n_filters: int, time_bins: int = TB):
    """Five clips' masks, built by hand: (bool (5, F), bool (5, time_bins), frontend.MaskPlan).  Clip 0: filter 0, the last
    filter and rows 30-34 where they exist (the 31/32 word boundary), time bins 60-70 (across a 64-bin piece); clips 1 and
    2: clear; clip 3: filters 63/64 (or the two middle rows), time bins 31/32 and the last bin; clip 4: time bins 0-9 only.
    EVERY clip's words also carry set bits at and beyond F / time_bins wherever the last word has room: they are ignored."""
    from lsm_speech_classifier_amd import frontend
    F = n_filters
    fm, tm = np.zeros((5, F), dtype=bool), np.zeros((5, time_bins), dtype=bool)
    fm[0, [0, F - 1]] = True
    fm[0, 30:min(35, F)] = True
    tm[0, 60:71] = True
    mid = 63 if F > 64 else F // 2
    fm[3, mid:mid + 2] = True
    tm[3, [31, 32, time_bins - 1]] = True
    tm[4, 0:10] = True
    freq, time = MR.words_of(fm), MR.words_of(tm)
    for words, bits in ((freq, F), (time, time_bins)):
        if bits & 31:
            words[:, -1] |= np.uint32((0xFFFFFFFF << (bits & 31)) & 0xFFFFFFFF)
    assert np.array_equal(MR.bits_of(freq, F), fm) and np.array_equal(MR.bits_of(time, time_bins), tm)
    return fm, tm, frontend.MaskPlan(freq, time)


def fused_audio():
    """Five clips for the fused tests: chirps of four classes and, third, a clip with a NaN sample."""
    from lsm_speech_classifier_amd import synth
    audio = synth.class_chirps([0, 5, 9, 3, 7], seed=31)
    audio[2, 7000] = np.nan
    return audio


# ---- split route ----------------------------------------------------------------------------------------------------------
def _split_call(torch, db, time_bins, thr, apply_floor, freq, time, masked=True, want_norm=True, red=2):
    lib = _lib_()
    f64 = db.dtype == np.float64
    dt = np.float64 if f64 else np.float32
    B, F, nc = db.shape
    on = np.array(sorted(thr, reverse=True), dtype=dt)
    off = np.array([dt(t - GAP) for t in sorted(thr, reverse=True)], dtype=dt)
    d = torch.from_numpy(db).cuda()
    raster = torch.full((B, F * red, time_bins * len(thr)), 7, dtype=torch.uint8, device="cuda")
    norm = torch.full((B, F, time_bins), -7.0, dtype=d.dtype, device="cuda") if want_norm else None
    args = [_p(d), B, F, nc, time_bins, apply_floor, _h(on), _h(off), len(on), red, _p(raster), _p(norm)]
    if masked:
        fn = lib.lsm_spec_to_spikes_masked_f64 if f64 else lib.lsm_spec_to_spikes_masked_f32
        rc = fn(*args, _p(freq), _p(time), None)
    else:
        fn = lib.lsm_spec_to_spikes_f64 if f64 else lib.lsm_spec_to_spikes_f32
        rc = fn(*args, None)
    assert rc == 0, lib.lsm_last_error().decode()
    torch.cuda.synchronize()
    return raster.cpu().numpy(), (norm.cpu().numpy() if want_norm else None)


def _walk_db(seed, B, F, nc, dtype):
    """Random-walk dB rows a few dozen dB wide: every threshold is crossed many times in both directions."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.standard_normal((B, F, nc)).cumsum(axis=2) * 4.0 - 30.0).astype(dtype))


def _split_masks(F, time_bins):
    """Three clips: clip 0 filter 0, 63/64 and 69, time bins 60-70 and 31/32; clip 1 clear; clip 2 the last bin and rows
    30-34; set bits beyond F and time_bins in every clip."""
    fm, tm = np.zeros((3, F), dtype=bool), np.zeros((3, time_bins), dtype=bool)
    fm[0, [0, 63, 64, F - 1]] = True
    tm[0, 60:71] = True
    tm[0, [31, 32]] = True
    fm[2, 30:35] = True
    tm[2, time_bins - 1] = True
    freq, time = MR.words_of(fm), MR.words_of(tm)
    freq[:, -1] |= np.uint32((0xFFFFFFFF << (F & 31)) & 0xFFFFFFFF)
    time[:, -1] |= np.uint32((0xFFFFFFFF << (time_bins & 31)) & 0xFFFFFFFF)
    return fm, tm, freq, time


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ncols,thr", [(98, THR), (100, THR8), (105, THR)])
def test_split_route_equals_the_restatement(torch_cuda, dtype, ncols, thr):
    """3 clips x 70 filters (two row groups of the encoder, three frequency words), redundancy 2; 98 and 105 columns are
    resized to 100 bins (105: the last bin is the zero bin), 100 are not."""
    F = 70
    db = _walk_db(ncols + len(thr), 3, F, ncols, dtype)
    fm, tm, freq, time = _split_masks(F, TB)
    assert (70 & 31) and (TB & 31) and freq.shape == (3, 3) and time.shape == (3, 4)
    zero_bin = ncols != TB and (TB - 1) * ((ncols - 1) / (TB - 1)) > ncols - 1      # the last bin lies outside the input
    assert zero_bin == (ncols == 105)
    raster, norm = _split_call(torch_cuda, db, TB, thr, 1, _words_dev(torch_cuda, freq), _words_dev(torch_cuda, time))
    want_norm, want = MR.masked_batch(db, TB, True, thr, GAP, 2, freq, time)
    assert norm.tobytes() == want_norm.tobytes()
    assert raster.tobytes() == want.tobytes()
    plain, plain_norm = _split_call(torch_cuda, db, TB, thr, 1, None, None, masked=False)
    assert raster[1].tobytes() == plain[1].tobytes() and norm[1].tobytes() == plain_norm[1].tobytes()     # the clear clip
    for b in (0, 2):
        assert raster[b].tobytes() != plain[b].tobytes()
        cells = fm[b][:, None] | tm[b][None, :]
        assert not norm[b][cells].view(np.uint64 if dtype == np.float64 else np.uint32).any()              # the bits of +0.0
        assert np.array_equal(norm[b][~cells], plain_norm[b][~cells])
    # one kind of mask at a time: the other pointer NULL
    only_f, _ = _split_call(torch_cuda, db, TB, thr, 1, _words_dev(torch_cuda, freq), None)
    only_t, _ = _split_call(torch_cuda, db, TB, thr, 1, None, _words_dev(torch_cuda, time))
    assert only_f.tobytes() == MR.masked_batch(db, TB, True, thr, GAP, 2, freq, None)[1].tobytes()
    assert only_t.tobytes() == MR.masked_batch(db, TB, True, thr, GAP, 2, None, time)[1].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_split_route_releases_the_latch_and_keeps_nan_clips_dark(torch_cuda, dtype):
    """The constructed case of tests/test_mask_host.py through the device: dB values 0.75, 0.65, ... beside a row 0, 1 with
    apply_floor = 0, threshold 0.7 / gap 0.1, bin 3 masked -- on for bins 0-2, then off for good; the unmasked raster with
    step 3 zeroed is on again from bin 4.  Second clip: the same with a NaN value -- masked cells are +0.0, the rest NaN,
    the raster stays all zeros."""
    Tb = 40
    db = np.full((2, 2, Tb), 0.65, dtype=dtype)
    db[:, 0, 0] = 0.75
    db[:, 1, :] = 0.0
    db[:, 1, 1] = 1.0
    db[1, 1, 7] = np.nan
    tm = np.zeros((2, Tb), dtype=bool)
    tm[:, 3] = True
    time = MR.words_of(tm)
    raster, norm = _split_call(torch_cuda, db, Tb, [0.7], 0, None, _words_dev(torch_cuda, time), red=1)
    want_norm, want = MR.masked_batch(db, Tb, False, [0.7], GAP, 1, None, time)
    assert raster.tobytes() == want.tobytes() and norm[0].tobytes() == want_norm[0].tobytes()
    # (the NaN clip: NaN where the restatement has NaN -- a NaN's sign and payload are no part of the definition)
    assert np.array_equal(np.isnan(norm[1]), np.isnan(want_norm[1])) and np.array_equal(norm[1][:, 3], want_norm[1][:, 3])
    assert raster[0, 0].tolist() == [1, 1, 1] + [0] * (Tb - 3)
    plain, _ = _split_call(torch_cuda, db, Tb, [0.7], 0, None, None, masked=False, red=1)
    assert MR.zeroed_raster(plain[0], 1, 1, None, tm[0])[0].tolist() == [1, 1, 1, 0] + [1] * (Tb - 4)
    assert not raster[1].any() and np.isnan(norm[1][:, :3]).all() and not norm[1][:, 3].any()


# ---- clear masks equal no masks -------------------------------------------------------------------------------------------
def test_clear_masks_equal_no_masks_in_all_four_entry_points(torch_cuda):
    """NULL pointers and zeroed word arrays, each against the unmasked twin, byte for byte."""
    from lsm_speech_classifier_amd import frontend, synth
    torch = torch_cuda
    for dtype in (np.float64, np.float32):
        db = _walk_db(5, 3, 70, 98, dtype)
        plain, plain_norm = _split_call(torch, db, TB, THR, 1, None, None, masked=False)
        zf, zt = torch.zeros((3, 3), dtype=torch.int32, device="cuda"), torch.zeros((3, 4), dtype=torch.int32, device="cuda")
        for freq, time in ((None, None), (zf, zt), (zf, None), (None, zt)):
            raster, norm = _split_call(torch, db, TB, THR, 1, freq, time)
            assert raster.tobytes() == plain.tobytes() and norm.tobytes() == plain_norm.tobytes()
    audio = synth.class_chirps([0, 5, 9], seed=31)
    for filterbank, F in (("gammatone", 40), ("mel", 40)):
        fe = frontend.SpikeFrontEnd(F, filterbank)
        plain = fe.encode(audio, fused=True)
        zero = frontend.MaskPlan(np.zeros((3, 2), dtype=np.uint32), np.zeros((3, 4), dtype=np.uint32))
        assert torch.equal(fe.encode(audio, fused=True, mask=zero), plain)
        assert torch.equal(fe.encode(audio, fused=False, mask=zero), plain)
        null = _fused_null(torch, fe, audio)                         # the masked entry point with both pointers NULL
        assert torch.equal(null, plain)


def _fused_null(torch, fe, audio):
    """The masked one-launch entry point of `fe` called with NULL masks (the Python layer never passes NULL)."""
    from lsm_speech_classifier_amd import frontend, mel as _mel
    lib = _lib_()
    x = torch.from_numpy(audio).cuda()
    B = len(audio)
    raster = torch.empty((B, fe.n_channels, fe.n_steps), dtype=torch.uint8, device="cuda")
    if fe.filterbank == "mel":
        m = fe._mel
        on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float32)
        ws = m.new_workspace(B)
        rc = lib.lsm_mel_spikes_masked_f32(
            _p(x), B, m.n_samples, _mel.N_FFT, m.hop, m.n_frames, _p(m.window), _p(m.twiddle), _p(m.basis), _p(m.lo), _p(m.hi),
            m.n_mels, C.c_float(_mel.AMIN), C.c_float(_mel.TOP_DB), fe.time_bins, _h(on), _h(off), len(on), fe.redundancy, _p(raster),
            _p(ws), int(ws.numel()), None, None, None)
    else:
        on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
        ws = fe.new_workspace(B)
        rc = lib.lsm_gammatone_spikes_masked_f64(
            _p(x), B, fe.n_samples, _p(fe.coefs), fe.n_filters, fe.nwin, fe.hop, fe.ncols, fe.time_bins, _h(on), _h(off),
            len(on), fe.redundancy, _p(raster), _p(ws), ws.numel() * 8, fe.coef_flags, 0, None, None, None)
    assert rc == 0, lib.lsm_last_error().decode()
    torch.cuda.synchronize()
    return raster


# ---- fused gammatone ------------------------------------------------------------------------------------------------------
LAYOUTS = [(40, "4", 0, 0), (128, "4", 0, 0), (200, "4", 0, 0),          # the lane pair (4 hardware queues)
           (128, "12", 1, 1), (320, "12", 1, 1),                          # one chain per lane (low-latency flag)
           (128, "12", 0, 2), (320, "12", 0, 2)]                          # two chains per lane


@pytest.mark.parametrize("n_filters,queues,flags,layout", LAYOUTS)
def test_fused_gammatone_equals_the_masked_split_route_and_the_restatement(torch_cuda, monkeypatch, n_filters, queues, flags,
                                                                           layout):
    """5 clips (the last workgroup has waves beyond the batch), one of them with a NaN sample; 1 to 5 waves per clip."""
    from lsm_speech_classifier_amd import frontend
    torch = torch_cuda
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
    lib = _lib_()
    assert lib.lsm_gammatone_spikes_layout(5, n_filters, flags) == layout
    audio = fused_audio()
    fe = frontend.SpikeFrontEnd(n_filters, "gammatone")
    fm, tm, plan = hand_masks(n_filters)
    fused = fe.encode(audio, fused=True, low_latency=bool(flags), mask=plan)
    db, _ = fe.spectrogram_db(audio)
    split, norm = fe.spikes_from_db(db, want_norm=True, mask=plan)
    assert torch.equal(fused, split)
    got = fused.cpu().numpy()
    db_host = db.cpu().numpy()
    want_norm, want = MR.masked_batch(db_host, TB, True, THR, GAP, fe.redundancy, plan.freq, plan.time)
    assert got.tobytes() == want.tobytes()
    got_norm = norm.cpu().numpy()                                   # (a NaN's sign and payload are no part of the definition)
    finite = ~np.isnan(want_norm)
    assert np.array_equal(np.isnan(got_norm), ~finite) and got_norm[finite].tobytes() == want_norm[finite].tobytes()
    assert np.isnan(want_norm[2]).all() and finite[[0, 1, 3, 4]].all()
    plain = fe.encode(audio, fused=True, low_latency=bool(flags)).cpu().numpy()
    # the NaN clip is dark, its neighbours and the clear clip are what they are without a mask in the batch
    assert not got[2].any() and not plain[2].any() and got[1].any() and got[1].tobytes() == plain[1].tobytes()
    # (a) every clip with a non-clear mask differs from its unmasked raster; (b) masking is not zeroing the raster
    differs_from_zeroed = []
    for b in range(5):
        if fm[b].any() or tm[b].any():
            assert got[b].tobytes() != plain[b].tobytes(), f"clip {b}: the mask changed nothing"
            zeroed = MR.zeroed_raster(plain[b], len(THR), fe.redundancy, fm[b], tm[b])
            differs_from_zeroed.append(got[b].tobytes() != zeroed.tobytes())
    assert len(differs_from_zeroed) == 3 and any(differs_from_zeroed)
    # the same masks moved to other clips: now the NaN clip has one -- still dark -- and the routes still agree
    moved = plan.take([1, 3, 0, 4, 2])
    fused2 = fe.encode(audio, fused=True, low_latency=bool(flags), mask=moved)
    assert torch.equal(fused2, fe.spikes_from_db(db, mask=moved)[0])
    got2 = fused2.cpu().numpy()
    assert got2.tobytes() == MR.masked_batch(db_host, TB, True, THR, GAP, fe.redundancy, moved.freq, moved.time)[1].tobytes()
    assert not got2[2].any() and got2[0].tobytes() == plain[0].tobytes()


def test_fused_gammatone_eight_thresholds_no_resize_and_redundancy(torch_cuda, monkeypatch):
    """The epilogue's other straight-line forms: 8 thresholds (two bins per field word), 40 columns for 40 bins (no
    resize, one live window), redundancy 3; lane pair and two chains."""
    from lsm_speech_classifier_amd import frontend, synth
    torch = torch_cuda
    x = synth.class_chirps([0, 5, 9, 3, 7], seed=31)
    n_samples = x.shape[1]
    for time_bins in (TB, 40):
        for queues, layout in (("4", 0), ("12", 2)):
            monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
            fe = frontend.SpikeFrontEnd(72, "gammatone", redundancy=3, thresholds=THR8, gap=0.02, n_samples=n_samples,
                                        time_bins=time_bins)
            assert _lib_().lsm_gammatone_spikes_layout(5, 72, 0) == layout and (fe.ncols == time_bins) == (time_bins == 40)
            _, _, plan = hand_masks(72, time_bins)
            fused = fe.encode(x, fused=True, mask=plan)
            db, _ = fe.spectrogram_db(x)
            assert torch.equal(fused, fe.spikes_from_db(db, mask=plan)[0])
            want = MR.masked_batch(db.cpu().numpy(), time_bins, True, THR8, 0.02, 3, plan.freq, plan.time)[1]
            assert fused.cpu().numpy().tobytes() == want.tobytes()
            assert not torch.equal(fused, fe.encode(x, fused=True))


# ---- mel one-launch -------------------------------------------------------------------------------------------------------
def test_mel_one_launch_equals_the_masked_split_route(torch_cuda):
    from lsm_speech_classifier_amd import frontend, synth
    torch = torch_cuda
    audio = synth.class_chirps([0, 5, 9, 3, 7], seed=31)
    fe = frontend.SpikeFrontEnd(40, "mel")
    fm, tm, plan = hand_masks(40)
    fused = fe.encode(audio, fused=True, mask=plan)
    split = fe.encode(audio, fused=False, mask=plan)
    assert torch.equal(fused, split)
    db, _ = fe.spectrogram_db(audio)
    want = MR.masked_batch(db.cpu().numpy(), TB, False, THR, GAP, fe.redundancy, plan.freq, plan.time)[1]
    assert split.cpu().numpy().tobytes() == want.tobytes()
    plain = fe.encode(audio, fused=True)
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    assert bool(fused.any()) and not torch.equal(fused, plain)      # (which clips a mask changes is the restatement's to say)


# ---- HotPath --------------------------------------------------------------------------------------------------------------
KEYS = ['spike_counts', 'mean_spike_times', 'mean_isi']


def _small_net(F):
    from lsm_speech_classifier_amd import reservoir as Rv, snn
    res = Rv.build_reservoir(Rv.SimulationParams(num_neurons=64, num_output_neurons=32, small_world_graph_k=8,
                                                 mean_weight=2.0 / 4, refractory_period=2), F)
    return snn.SNN(None, reservoir=res)


@pytest.mark.parametrize("topology", ["serial", "two-stage"])
def test_hotpath_masks_inside_the_front_end(torch_cuda, topology):
    from lsm_speech_classifier_amd import frontend, pipeline, synth
    torch = torch_cuda
    streams = 1 if topology == "serial" else pipeline.DEFAULT_STREAMS
    audio = synth.class_chirps([0, 5, 9, 3, 7], seed=31)
    F = 40
    fe, net = frontend.SpikeFrontEnd(F, "gammatone"), _small_net(F)
    _, _, plan = hand_masks(F)
    noise = synth.coloured_noise(2, 4097, seed=4).astype(np.float32)
    mixer = frontend.NoiseMixer(noise)
    mix = frontend.mix_plan(5, 2, 4097, 10.0, seed=9)
    hp = pipeline.HotPath(fe, net, KEYS, streams=streams, mixer=mixer)
    if topology == "two-stage":
        assert hp.n_fe_streams and fe.will_fuse()

    def rows_of(x, **plans):
        feats, st = hp.submit(x, **plans)
        st.synchronize()
        return feats.cpu().numpy().tobytes()

    def direct(x, mask=None):
        feats = net.run_batch(fe.encode(x, mask=mask) if mask is not None else fe.encode(x), KEYS)[0]
        torch.cuda.synchronize()
        return feats.cpu().numpy().tobytes()

    masked, clean = direct(audio, plan), direct(audio)
    assert masked != clean
    assert rows_of(audio, mask=plan) == masked
    assert rows_of(audio) == clean                                   # the next step, without a mask
    assert rows_of(audio, mask=plan) == masked
    # corruption first, the mask inside the front end
    noisy = mixer.mix(torch.from_numpy(audio).cuda(), *mix)
    assert rows_of(audio, mix=mix, mask=plan) == direct(noisy, plan) != masked
    # run(masks=...) and features_from_audio slice the plan per batch
    got = hp.run([audio[0:2], audio[2:4], audio[4:5]], masks=[plan.part(0, 2), plan.part(2, 4), plan.part(4, 5)])
    assert got.cpu().numpy().tobytes() == masked
    assert hp.run([audio[0:2], audio[2:5]]).cpu().numpy().tobytes() == clean
    feats = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, mask=plan)
    assert feats.tobytes() == masked
    assert pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams).tobytes() == clean
    with pytest.raises(ValueError, match="mask plan covers"):
        pipeline.features_from_audio(audio, fe, net, KEYS, mask=plan.part(0, 2))
    with pytest.raises(ValueError):
        hp.submit(audio, mask=plan.part(0, 3))
    with pytest.raises(ValueError, match="front end"):
        hp.submit(fe.encode(audio), stage="reservoir", mask=plan)
    hp.synchronize()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_the_twins_first_then_the_misaligned_mask(torch_cuda):
    from lsm_speech_classifier_amd import frontend, mel as _mel, synth
    torch = torch_cuda
    lib = _lib_()
    B, F, nc = 2, 8, 98
    db = torch.from_numpy(_walk_db(1, B, F, nc, np.float64)).cuda()
    on, off = np.array([0.7]), np.array([0.6])
    raster = torch.full((B, F, TB), 9, dtype=torch.uint8, device="cuda")
    words = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    msg = lambda: lib.lsm_last_error().decode()

    def split(fn=lib.lsm_spec_to_spikes_masked_f64, d=db, n_thr=1, red=1, freq=None, time=None, nf=F):
        return fn(_p(d), B, nf, nc, TB, 1, _h(on), _h(off), n_thr, red, _p(raster), None, _p(freq), _p(time), None)

    assert split(freq=words.data_ptr() + 2) == -1 and re.search("freq_mask and time_mask must be 4-byte aligned", msg())
    assert split(time=words.data_ptr() + 1) == -1 and re.search("4-byte aligned", msg())
    assert split(freq=words.data_ptr() + 2, fn=lib.lsm_spec_to_spikes_masked_f32,
                 d=db.float()) == -1 and re.search("4-byte aligned", msg())
    # the twin's refusals come first, in the twin's order, with the twin's words
    bad = words.data_ptr() + 2
    for kw, text in ((dict(nf=0), "bad shape"), (dict(d=None), "null input"), (dict(n_thr=9), r"n_thr=9 outside \[0, 8\]"),
                     (dict(red=0), "redundancy must be >= 1"), (dict(nf=0, n_thr=9, red=0), "bad shape"),
                     (dict(n_thr=9, red=0), "n_thr=9"), (dict(n_thr=0), "a raster needs at least one threshold")):
        assert split(freq=bad, **kw) == -1 and re.search(text, msg()), (kw, msg())
        unmasked = lib.lsm_spec_to_spikes_f64(_p(kw.get("d", db)), B, kw.get("nf", F), nc, TB, 1, _h(on), _h(off),
                                              kw.get("n_thr", 1), kw.get("red", 1), _p(raster), None, None)
        assert unmasked == -1 and re.search(text, msg())
    # the fused launches
    audio = torch.from_numpy(synth.class_chirps([0, 5], seed=31)).cuda()
    fe = frontend.SpikeFrontEnd(8, "gammatone")
    on4, off4 = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
    ws = fe.new_workspace(B)
    r4 = torch.full((B, 8, 400), 9, dtype=torch.uint8, device="cuda")

    def fused(freq=None, time=None, ws_bytes=None, flags=0, nf=8):
        return lib.lsm_gammatone_spikes_masked_f64(
            _p(audio), B, fe.n_samples, _p(fe.coefs), nf, fe.nwin, fe.hop, fe.ncols, fe.time_bins, _h(on4), _h(off4), 4, 1,
            _p(r4), _p(ws), ws.numel() * 8 if ws_bytes is None else ws_bytes, fe.coef_flags, flags, _p(freq), _p(time), None)

    assert fused(freq=bad) == -1 and re.search("4-byte aligned", msg())
    assert fused(time=bad) == -1 and re.search("4-byte aligned", msg())
    assert fused(freq=bad, flags=4) == -1 and re.search("launch_flags", msg())
    assert fused(freq=bad, nf=1) == -1 and re.search("n_filters >= 2", msg())
    assert fused(freq=bad, ws_bytes=8) == -1 and re.search("workspace of 8 bytes", msg())
    fm = frontend.SpikeFrontEnd(8, "mel")
    m = fm._mel
    on32, off32 = frontend.threshold_tables(fm.thresholds, fm.gap, np.float32)
    mws = m.new_workspace(B)

    def mel(freq=None, time=None, n_fft=2048):
        return lib.lsm_mel_spikes_masked_f32(
            _p(audio), B, m.n_samples, n_fft, m.hop, m.n_frames, _p(m.window), _p(m.twiddle), _p(m.basis), _p(m.lo), _p(m.hi),
            m.n_mels, C.c_float(_mel.AMIN), C.c_float(_mel.TOP_DB), TB, _h(on32), _h(off32), 4, 1, _p(r4), _p(mws), int(mws.numel()),
            _p(freq), _p(time), None)

    assert mel(time=bad) == -1 and re.search("4-byte aligned", msg())
    assert mel(time=bad, n_fft=1024) == -1 and re.search("n_fft must be 2048", msg())
    torch.cuda.synchronize()
    assert bool((raster == 9).all()) and bool((r4 == 9).all()), "a refused call wrote"
    # the calls the refusals start from
    assert split(freq=words, time=words) == 0 and fused(freq=words, time=words) == 0, msg()
    torch.cuda.synchronize()
    assert not bool((raster == 9).any()) and not bool((r4 == 9).any())
    assert mel(freq=words, time=words) == 0, msg()
    torch.cuda.synchronize()
