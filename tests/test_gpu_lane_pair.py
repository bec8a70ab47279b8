"""The lane-pair layout of the one-launch gammatone front end (`lsm_gammatone_spikes_f64`, 2..256 filters in batches
that the two-chain layout would not spread over the whole chip: channel j of a 32-channel group in lanes j and j + 32,
sections 1-2 on the first lane, 3-4 one sample later on the second) against the C oracle and the split entry points
(`gammatone_kernel` -> `spec_to_spikes`).  Reference: /root/reference/create_dataset.py:49-104."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = [0.70, 0.80, 0.90, 0.95]
GAP = 0.1
THR8 = [0.3, 0.6, 0.65, 0.7, 0.8, 0.9, 0.95, 0.99]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


@pytest.fixture(autouse=True)
def scarce_queues(monkeypatch):
    """The library takes the lane pair only with at most 4 hardware queues (GPU_MAX_HW_QUEUES, read at every launch);
    these tests ask for it whatever the process really has -- the queue count changes the layout, never a result."""
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    return monkeypatch


def _layout(n_clips, n_filters, flags=0):
    from lsm_speech_classifier_amd import _lib
    return _lib.load().lsm_gammatone_spikes_layout(n_clips, n_filters, flags)


def _oracle_raster(oracle_c, audio, fe, thr=THR, gap=GAP):
    coefs = fe.coefs.cpu().numpy()
    with np.errstate(all="ignore"):
        return np.stack([oracle_c.encode_hysteresis(oracle_c.normalise_resize(oracle_c.gammatone_db(
            oracle_c.gammatone_spec(a, coefs, fe.nwin, fe.hop, fe.ncols)), fe.time_bins), thr, gap) for a in audio])


def _routes_agree(torch_cuda, fe, audio, monkeypatch):
    """The fused launch in the lane pair equals the split launches and the fused launch in the one- and two-chain
    layouts (what 12 queues select); returns the lane pair's raster."""
    pair = fe.n_filters <= 256
    assert _layout(len(audio), fe.n_filters) == (0 if pair else 2)
    fused = fe.encode(audio, fused=True)
    assert torch_cuda.equal(fused, fe.encode(audio, fused=False))
    with monkeypatch.context() as m:
        m.setenv("GPU_MAX_HW_QUEUES", "12")
        assert _layout(len(audio), fe.n_filters, 1) == (1 if fe.n_filters <= 512 else 2)
        assert torch_cuda.equal(fused, fe.encode(audio, fused=True, low_latency=True))
        if fe.n_filters > 64:
            assert _layout(len(audio), fe.n_filters) == 2
            assert torch_cuda.equal(fused, fe.encode(audio, fused=True))
    return fused.cpu().numpy()


@pytest.mark.parametrize("n_filters", [2, 31, 32, 33, 64, 65, 127, 128, 200, 256, 257])
def test_lane_pair_filter_counts(torch_cuda, oracle_c, n_filters, scarce_queues):
    """One to eight waves per clip, ragged last 32-channel group, 257 = the first count past the lane pair; five clips:
    the last workgroup is partly empty wherever a workgroup holds more than one clip."""
    from lsm_speech_classifier_amd import frontend, synth
    audio = np.concatenate([synth.class_chirps([0, 5, 9], seed=31), synth.white_noise(2, seed=9)])
    audio[3] = 0.0                                            # silent clip: flat spectrogram -> zeros
    fe = frontend.SpikeFrontEnd(n_filters, "gammatone")
    got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
    assert got.shape == (len(audio), n_filters, 400)
    assert not got[3].any() and got.sum() > 0
    np.testing.assert_array_equal(got, _oracle_raster(oracle_c, audio, fe))


@pytest.mark.parametrize("n_samples,time_bins,nw", [(48000, 100, 1), (16000, 40, 1), (24000, 100, 2), (16000, 100, 3),
                                                    (12345, 77, 3), (12000, 100, 4), (13000, 100, 4)])
@pytest.mark.parametrize("n_filters", [33, 128])
def test_lane_pair_window_overlaps(torch_cuda, oracle_c, n_samples, time_bins, nw, n_filters, scarce_queues):
    """NW = 1..4 overlapping windows, hops that are not multiples of 8, no resize (40 columns, 40 bins); the head lane
    reads one sample ahead of the tail, up to the clip's last sample."""
    from lsm_speech_classifier_amd import frontend, synth
    rng = np.random.RandomState(n_samples + time_bins + n_filters)
    base = synth.class_chirps([2, 6, 10], seed=8)
    audio = np.ascontiguousarray(np.resize(base, (3, n_samples)).astype(np.float32))
    audio += 0.01 * rng.randn(3, n_samples).astype(np.float32)
    fe = frontend.SpikeFrontEnd(n_filters, "gammatone", n_samples=n_samples, time_bins=time_bins)
    assert (fe.nwin + fe.hop - 1) // fe.hop == nw
    got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
    np.testing.assert_array_equal(got, _oracle_raster(oracle_c, audio, fe))


def test_lane_pair_clip_ending_on_a_window(torch_cuda, oracle_c, scarce_queues):
    """The last column ends on the clip's last sample (n_end == n_samples): the head lane's look-ahead is clamped."""
    from lsm_speech_classifier_amd import frontend, synth
    n = 10000                                                 # hop 100, 97 columns: 96 * 100 + 400 samples
    audio = np.ascontiguousarray(synth.class_chirps([1, 7], seed=4)[:, :n])
    fe = frontend.SpikeFrontEnd(64, "gammatone", n_samples=n, time_bins=100)
    assert (fe.ncols - 1) * fe.hop + fe.nwin == n
    got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
    np.testing.assert_array_equal(got, _oracle_raster(oracle_c, audio, fe))


@pytest.mark.parametrize("n_filters", [32, 128, 200])
def test_lane_pair_nan_and_inf_clips(torch_cuda, oracle_c, n_filters, scarce_queues):
    """A NaN or +-Inf sample makes its clip's raster all zeros (NaN max / min, create_dataset.py:59-63); the other clips
    of the batch, in the same workgroup or not, are untouched."""
    from lsm_speech_classifier_amd import frontend, synth
    audio = np.concatenate([synth.class_chirps([0, 4, 8, 11], seed=2), synth.white_noise(3, seed=6)])
    audio[1, 7000] = np.nan
    audio[2, 0] = np.inf
    audio[4, 15999] = -np.inf
    audio[5, 8] = np.nan
    fe = frontend.SpikeFrontEnd(n_filters, "gammatone")
    got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
    ref = _oracle_raster(oracle_c, audio, fe)
    assert not ref[1].any() and not ref[2].any() and not ref[5].any() and ref[0].any() and ref[6].any()
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("n_filters", [31, 96, 128])
def test_lane_pair_redundancy_and_eight_thresholds(torch_cuda, oracle_c, n_filters, scarce_queues):
    from lsm_speech_classifier_amd import frontend, synth
    audio = synth.class_chirps([1, 4, 9], seed=3)
    for red, thr, gap in ((3, THR, GAP), (2, THR8, 0.02), (1, THR8, 0.05)):
        fe = frontend.SpikeFrontEnd(n_filters, "gammatone", redundancy=red, thresholds=thr, gap=gap)
        got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
        ref = np.repeat(_oracle_raster(oracle_c, audio, fe, thr=thr, gap=gap), red, axis=1)
        np.testing.assert_array_equal(got, ref)


def test_lane_pair_general_coefficients(torch_cuda, oracle_c, scarce_queues):
    """A table without the shared first-section gain or the zero b2 products (coef_flags 0): the general
    two-section code (true division, b2 * x terms) on both halves of the pair."""
    from lsm_speech_classifier_amd import frontend, synth
    audio = synth.class_chirps([3, 8, 10], seed=12)
    fe = frontend.SpikeFrontEnd(96, "gammatone")
    tab = fe.coefs.cpu().numpy().copy()
    tab[:, 0] *= 1.0 + 1e-3 * np.arange(96)                  # channel-dependent A0
    tab[:, 5] = 1e-9 * tab[:, 0]                             # non-zero A2: the x*b2 products count
    fe.coefs = torch_cuda.from_numpy(tab).cuda()
    fe.coef_flags = frontend.coef_flags(tab) & ~1
    assert (fe.coef_flags & 1) == 0
    got = _routes_agree(torch_cuda, fe, audio, scarce_queues)
    np.testing.assert_array_equal(got, _oracle_raster(oracle_c, audio, fe))


def test_lane_pair_equals_two_chain_layout_of_a_full_chip_batch(torch_cuda):
    """1024 clips x 128 filters fill the chip in the two-chain layout and keep it; the same clips in small batches take
    the lane pair.  Both layouts give the same rasters, whatever the position of a clip in its batch."""
    from lsm_speech_classifier_amd import frontend, synth
    audio = synth.class_chirps(np.arange(1030) % 12, seed=55)
    fe = frontend.SpikeFrontEnd(128, "gammatone")
    dev = torch_cuda.from_numpy(audio).cuda()
    big = fe.encode(dev, fused=True)
    for lo, hi in ((0, 256), (256, 259), (1021, 1030)):
        assert torch_cuda.equal(big[lo:hi], fe.encode(dev[lo:hi], fused=True))
        assert torch_cuda.equal(big[lo:hi], fe.encode(dev[lo:hi], fused=True, low_latency=True))


def test_layout_selection(torch_cuda, scarce_queues):
    """The lane pair for 2..256 filters with at most 4 hardware queues, either value of the low-latency flag; the chain
    layouts with more queues, above 256 filters, and for a batch that fills every SIMD in the two-chain layout."""
    for F in (2, 32, 128, 256):
        assert _layout(256, F) == 0 and _layout(256, F, 1) == 0 and _layout(3, F, 2) == 0
    assert _layout(256, 257) == 2 and _layout(256, 257, 1) == 1 and _layout(256, 1024, 1) == 2
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert _layout(4 * cus, 128) == 2 and _layout(4 * cus - 1, 128) == 0 and _layout(2 * cus, 256) == 2
    assert _layout(256, 1025) < 0 and _layout(0, 128) < 0
    scarce_queues.setenv("GPU_MAX_HW_QUEUES", "12")
    assert _layout(256, 128) == 2 and _layout(256, 128, 1) == 1 and _layout(256, 40) == 1
    scarce_queues.delenv("GPU_MAX_HW_QUEUES")                   # the runtime's default: 4
    assert _layout(256, 128) == 0
