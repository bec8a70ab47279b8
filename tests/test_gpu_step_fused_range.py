"""The one-launch step (`lsm_step_fused_f64`) over the range it serves: all six kernel forms (1, 2 and 4 neuron slots per
lane, with and without the shared first-section gain), the edges of the hand-off of the staged raster bits into the
reservoir's input rows (one word, an even and an odd number of words, a partial and a full last word, 1 to 8 thresholds),
waves that own no neurons, the launch with more than 64 KB of LDS up to the bound of 160 KB, more clips than compute units,
and both sides of every boundary of `lsm_step_fused_supported`.  Every case is compared bit for bit with the C oracle
(front end and reservoir), with the two launches it replaces and, in `stats_out`, with the oracle's spike matrix.

Inputs: `n_samples = time_bins * hop`, the clips are two class chirps and one white-noise clip, the thresholds are
`(i + 1) / (n_thr + 1)` rounded to 4 places, the reservoir is built as in test_gpu_step_fused.py."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LDS_MAX = 160 * 1024
_built = {}


def _thresholds(n_thr):
    return [round((i + 1) / (n_thr + 1), 4) for i in range(n_thr)]


def _clips(n_samples):
    from lsm_speech_classifier_amd import synth
    return np.ascontiguousarray(np.concatenate([synth.class_chirps([0, 5], seed=31, n_samples=n_samples),
                                                synth.white_noise(1, seed=9, n_samples=n_samples)]), dtype=np.float32)


def _oracle_raster(oracle_c, fe, tab, clip):
    with np.errstate(all="ignore"):
        return oracle_c.encode_hysteresis(oracle_c.normalise_resize(oracle_c.gammatone_db(
            oracle_c.gammatone_spec(clip, tab, fe.nwin, fe.hop, fe.ncols)), fe.time_bins), fe.thresholds, fe.gap)


def _front_end(F, bins, n_thr, hop):
    from lsm_speech_classifier_amd import frontend
    fe = frontend.SpikeFrontEnd(F, "gammatone", thresholds=_thresholds(n_thr), time_bins=bins, n_samples=bins * hop)
    assert (fe.nwin, fe.hop, fe.n_steps) == (400, hop, bins * n_thr) and fe.coef_flags == 7
    return fe


def _reservoir(N, channels, rasters):
    """The existing test's reservoir: k = N / 5, 2 N / 5 output neurons, the critical weight of the given rasters."""
    from lsm_speech_classifier_amd import reservoir as R, snn
    from oracle import ref_numpy as O
    k = N // 5
    p = R.SimulationParams(num_neurons=N, num_output_neurons=2 * N // 5, small_world_graph_k=k,
                           mean_weight=O.w_critico(k, 2.0, 2, rasters) * 1.0)
    return snn.SNN(None, reservoir=R.build_reservoir(p, channels))


def _build(oracle_c, F, bins, n_thr, hop, N):
    """Front end, reservoir (its weight from the oracle's rasters of the two chirps) and the three clips of a shape, built
    once; the tests leave them as they are."""
    key = (F, bins, n_thr, hop, N)
    if key not in _built:
        fe = _front_end(F, bins, n_thr, hop)
        audio = _clips(bins * hop)
        tab = fe.coefs.cpu().numpy()
        net = _reservoir(N, F, np.stack([_oracle_raster(oracle_c, fe, tab, a) for a in audio[:2]]))
        _built[key] = fe, net, audio
    return _built[key]


def _slots_per_lane(N):
    sl = 1
    while 4 * 64 * sl < N:
        sl *= 2
    return sl


def _max_wave_spikes(sm, N):
    """The most spikes one producer wave of the 4-wave layout has in one step."""
    per = 64 * _slots_per_lane(N)
    return max(int(sm[:, w * per:(w + 1) * per].sum(axis=1).max()) for w in range(4) if w * per < N)


def _check(oracle_c, fe, net, audio, oracle_clips=None, nonempty=2, keys=None, fused=None):
    """The fused step on `audio` against the two launches (rows and stats_out, every clip) and the C oracle (rows, and
    stats_out against the spike matrix; the clips `oracle_clips`, default all).  At least `nonempty` of the oracle's clips
    must have input spikes and reservoir spikes.  `fused`: `encode`'s (False: the split front-end launches).  Returns the rows, the oracle's spike matrices and the rasters."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    from lsm_speech_classifier_amd.snn import FEATURE_KEYS
    B, N, T = len(audio), net.reservoir.num_neurons, fe.n_steps
    plan = net.plan(B, T, -1)
    assert (plan["kernel"], plan["waves_per_clip"], plan["slots_per_lane"]) == ("dense", 4, _slots_per_lane(N)), plan
    assert pipeline.step_fused_supported(fe, net, B)
    x = torch.from_numpy(audio).cuda()
    stats = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    got = pipeline.step_fused(fe, net, x, keys, stats_out=stats)
    torch.cuda.synchronize()
    assert got.shape == (B, len(keys or FEATURE_KEYS) * net.num_output_neurons)
    stats2 = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    rasters = fe.encode(x, fused=fused)
    want = net.run_batch(rasters, keys, stats_out=stats2, waves_per_clip=-1)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want), "rows differ from run_batch(encode(x))"
    assert torch.equal(stats, stats2), "stats_out differs from the two launches'"
    rows, st, rasters = got.cpu().numpy(), stats.cpu().numpy(), rasters.cpu().numpy()
    tab = fe.coefs.cpu().numpy()
    sms, live = {}, 0
    for b in range(B) if oracle_clips is None else oracle_clips:
        raster = _oracle_raster(oracle_c, fe, tab, audio[b])
        np.testing.assert_array_equal(raster, rasters[b])
        feats, sm, _ = oracle_c.lif_run(net.reservoir, raster, keys)
        np.testing.assert_array_equal(rows[b], feats.reshape(-1), err_msg=f"clip {b}")
        assert st[b].tolist() == [int(sm.any(axis=0).sum()), int(sm.sum())], f"clip {b}: stats_out"
        live += bool(raster.any() and sm.any())
        sms[b] = sm
    assert live >= nonempty, f"{live} clips with input and reservoir spikes"
    return got, sms, rasters


# 1. all six forms: 1, 2 and 4 slots per lane x the shared and the channel-dependent first-section gain

@pytest.mark.parametrize("N", [256, 384, 1000])
def test_every_kernel_form_equals_the_oracle(oracle_c, N):
    """F = 128, 16 bins x 4 thresholds on hop 160 (T = 64).  The stock table (coef_flags 7) and a table with a
    channel-dependent A0 (coef_flags 3) on the same reservoir; the two tables' rows differ, and so do the rows of the second
    table under a claimed coef_flags 7: the bit selects the kernel.  With 2 slots per lane the batch also holds a silent clip
    and a clip with one NaN sample (no input spike: a flat and a NaN spectrogram)."""
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net, audio = _build(oracle_c, 128, 16, 4, 160, N)
    assert net.plan(len(audio), 64, -1)["slots_per_lane"] == {256: 1, 384: 2, 1000: 4}[N]
    oracle_clips = None
    if N == 384:
        audio = np.concatenate([audio, audio[:2]])
        audio[3] = 0.0
        audio[4, 1000] = np.nan
        oracle_clips = range(5)
    stock, sms, rasters = _check(oracle_c, fe, net, audio, oracle_clips)
    if N == 384:
        assert not rasters[3:].any() and not sms[3].any() and not sms[4].any()
    tab = fe.coefs.cpu().numpy().copy()
    tab[:, 0] *= 1.0 + 1e-3 * np.arange(128)                 # channel-dependent A0
    fe3 = _front_end(128, 16, 4, 160)
    fe3.coefs = torch.from_numpy(tab).cuda()
    fe3.coef_flags = frontend.coef_flags(tab)
    assert fe3.coef_flags == 3
    got = _check(oracle_c, fe3, net, audio, oracle_clips)[0]
    assert not torch.equal(got, stock)
    fe3.coef_flags = 7                                       # lying about the table must change the result: the bit is used
    assert not torch.equal(pipeline.step_fused(fe3, net, torch.from_numpy(audio).cuda()), got)


# 2. the edges of the hand-off and of the served range: (F, bins, n_thr, hop, N), T = bins * n_thr, RW = ceil(T / 32)

EDGES = [
    (128, 4, 1, 160, 100),      # T = 4, RW 1: the smallest shape the front end accepts (ncols = 2)
    (128, 5, 4, 160, 100),      # T = 20, RW 1: one partial word, waves 2 / 3 idle in the hand-off and in the reservoir
    (97, 32, 1, 160, 257),      # T = 32 exactly, 2 slots per lane, one neuron in wave 2, none in wave 3
    (128, 33, 1, 160, 300),     # T = 33, RW 2: the last word holds 1 bit and belongs to waves 2 / 3
    (113, 16, 4, 160, 512),     # T = 64, RW 2: full last word, 2 slots per lane full, F between the tested ends
    (127, 9, 7, 160, 513),      # T = 63: 7 thresholds (8-bit half fields), 31-bit tail, 4 slots with one neuron in wave 2
    (128, 12, 8, 160, 768),     # T = 96, RW 3: MAX_THR, odd RW, exact multiple of 32
    (97, 100, 3, 160, 1024),    # T = 300, RW 10: the largest served N, even RW, 12-bit tail
    (128, 10, 4, 134, 300),     # T = 40: the smallest hop with 3 live windows
    (128, 10, 4, 199, 300),     # T = 40: the largest hop with 3 live windows
    (128, 100, 4, 160, 64),     # T = 400, RW 13: all neurons in wave 0
]
# more than the 16 fixed list slots of spikes of one producer wave in one step (the merge path of the spike exchange) must
# occur in these cases: with 2 and with 4 slots per lane
# (oracle on the CPU: 18, 21, 22, 24 and 47 spikes)
MERGE = [(97, 32, 1, 160, 257), (128, 33, 1, 160, 300), (127, 9, 7, 160, 513), (128, 12, 8, 160, 768), (97, 100, 3, 160, 1024)]
CHIRPS_ONLY = [(97, 32, 1, 160, 257)]                         # clips: chirps 9, 0 and 5 (the stock clips reach 12 spikes)


@pytest.mark.parametrize("F,bins,n_thr,hop,N", EDGES)
def test_hand_off_edges_equal_the_oracle(oracle_c, F, bins, n_thr, hop, N):
    """Three clips, all 8 feature keys.  The first case runs 4 steps, too few for a reservoir spike: it checks rows and
    stats and is exempt from the non-empty condition on the spike matrix (its rasters are not empty)."""
    shape = (F, bins, n_thr, hop, N)
    fe, net, audio = _build(oracle_c, *shape)
    if shape in CHIRPS_ONLY:
        from lsm_speech_classifier_amd import synth
        audio = np.ascontiguousarray(synth.class_chirps([9, 0, 5], seed=31, n_samples=bins * hop))
    assert len(audio) == 3 and (nw := -(-fe.nwin // fe.hop)) == 3, nw
    tiny = bins * n_thr == 4
    sms = _check(oracle_c, fe, net, audio, nonempty=0 if tiny else 3)[1]
    if tiny:
        tab = fe.coefs.cpu().numpy()
        assert all(_oracle_raster(oracle_c, fe, tab, a).any() for a in audio)
    if shape in MERGE:
        assert max(_max_wave_spikes(sm, N) for sm in sms.values()) > 16


# 3. the LDS bound and the launch with more than 64 KB of LDS

def _lds_bytes(bins, n_thr, N, n_out):
    """the front end's exchange doubles (128 bytes) and staged raster rows (4 waves x 32 rows x RW words), then
    the dense-row reservoir's image (float32 accumulators and two uint16 step lists per padded neuron, 512 bytes of counts,
    16 bytes of feature accumulators per output neuron, 4 input words per step), then 128 bytes of inverse permutation."""
    T = bins * n_thr
    npad = 4 * 64 * _slots_per_lane(N)
    return 128 + 4 * 32 * -(-T // 32) * 4 + (4 * npad + 2 * 2 * npad + 512 + 16 * n_out + 4 * 4 * T) + 128


def _bound_shape(N=256):
    """F = 128, 4 thresholds, hop 160, N = 256: a reservoir of that size and `served(bins)`, host work only."""
    from lsm_speech_classifier_amd import pipeline
    if "bound" not in _built:
        _built["bound"] = _reservoir(N, 128, np.zeros((1, 128, 8), dtype=np.uint8))
    net = _built["bound"]
    return net, lambda bins: pipeline.step_fused_supported(_front_end(128, bins, 4, 160), net, 2)


def _largest_served_bins(served):
    lo, hi = 100, 16383                                      # 16383 x 4 = 65532 steps: the record limit is not the bound
    assert served(lo) and not served(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if served(mid) else (lo, mid)
    return lo


def test_the_lds_bound_is_the_documented_formula():
    """Bisection over time_bins on the host (no launch): the last served shape is the last whose restated LDS image fits
    160 KB, 1242 bins (T = 4968: 163 808 bytes; 1243 bins: 163 872)."""
    net, served = _bound_shape()
    n_out = net.num_output_neurons
    assert n_out == 102
    best = _largest_served_bins(served)
    assert _lds_bytes(best, 4, 256, n_out) <= LDS_MAX < _lds_bytes(best + 1, 4, 256, n_out)
    assert best == 1242 and _lds_bytes(1242, 4, 256, n_out) == 159360 + 4448


def test_two_clips_at_the_lds_bound_equal_the_oracle(oracle_c):
    """1242 bins x 4 thresholds (T = 4968, 198 720 samples a clip, 163 808 bytes of LDS), against the oracle and the
    reservoir launch on the rasters of the split front-end launches: `encode`'s one launch does not serve this row length
    with the suite's 12 hardware queues (its two-chain layout stages 64 rows per wave, 319 616 bytes)."""
    t0 = time.perf_counter()
    fe, net, audio = _build(oracle_c, 128, 1242, 4, 160, 256)
    assert _lds_bytes(1242, 4, 256, net.num_output_neurons) <= LDS_MAX
    _check(oracle_c, fe, net, audio[:2], fused=False)
    print(f"\nLDS bound case: {time.perf_counter() - t0:.1f} s wall")


def test_big_lds_launch_first_then_in_a_graph(oracle_c):
    """500 bins x 4 thresholds (T = 2000, 68 704 bytes of LDS): the first launch of a fresh front end and reservoir, then one
    capture after a warm-up launch, replayed on other audio in the captured buffer."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    fe, net, audio = _build(oracle_c, 128, 500, 4, 160, 256)
    assert 64 * 1024 < _lds_bytes(500, 4, 256, net.num_output_neurons) < LDS_MAX
    got = _check(oracle_c, fe, net, audio)[0]
    x = torch.from_numpy(audio[[2, 0, 1]]).cuda()
    out = torch.zeros_like(got)
    ws = fe.new_workspace(3)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        pipeline.step_fused(fe, net, x, features_out=out, workspace=ws)       # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            pipeline.step_fused(fe, net, x, features_out=out, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(out, got[[2, 0, 1]])
    x.copy_(torch.from_numpy(audio[[1, 2, 0]]).cuda())
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, got[[1, 2, 0]])


# 4. where lsm_step_fused_supported and the launch must agree

def _refused(fe, net, n_clips=1, says=""):
    """`supported` answers no and the launch raises LSM_ERR_UNSUPPORTED (-4) with a message that holds `says`."""
    import torch
    from lsm_speech_classifier_amd import _lib, pipeline
    assert not pipeline.step_fused_supported(fe, net, n_clips)
    x = torch.zeros((n_clips, fe.n_samples), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.LsmHipError, match=r"\(-4\).*" + says):
        pipeline.step_fused(fe, net, x)


@pytest.mark.parametrize("hop,served_hop", [(133, 134), (200, 199)])
def test_four_and_two_live_windows_are_refused(oracle_c, hop, served_hop):
    """10 bins on hop 133 (4 live windows of 400 samples) and on hop 200 (2); the served neighbours run in EDGES."""
    from lsm_speech_classifier_amd import pipeline
    fe, net, _ = _build(oracle_c, 128, 10, 4, served_hop, 300)
    assert (128, 10, 4, served_hop, 300) in EDGES and pipeline.step_fused_supported(fe, net, 1)
    _refused(_front_end(128, 10, 4, hop), net, says="make the two launches")


def test_eight_waves_per_clip_are_refused(oracle_c):
    """N = 1025 takes 8 waves per clip; N = 1024, the largest with 4, runs in EDGES."""
    assert (97, 100, 3, 160, 1024) in EDGES
    fe, _, _ = _build(oracle_c, 97, 100, 3, 160, 1024)
    net = _reservoir(1025, 97, np.zeros((1, 97, 8), dtype=np.uint8))
    assert net.plan(1, fe.n_steps, -1)["waves_per_clip"] == 8
    _refused(fe, net)


def test_another_channel_count_is_refused(oracle_c):
    """A 128-filter front end with the reservoir of a 97-filter one (which the 97-filter front end runs in EDGES)."""
    _, net97, _ = _build(oracle_c, 97, 32, 1, 160, 257)
    _refused(_front_end(128, 32, 1, 160), net97)


def test_one_past_the_lds_bound_is_refused():
    """1243 bins at the shape of the bound: 64 bytes too many; the launch says UNSUPPORTED, not a bad argument."""
    net, served = _bound_shape()
    assert served(1242)
    _refused(_front_end(128, 1243, 4, 160), net, 2, says="163872 bytes.*make the two launches")


def test_more_steps_than_the_records_hold_are_refused():
    """8192 bins x 8 thresholds = 65536 steps, one more than the reservoir's 16-bit spike times hold."""
    net, _ = _bound_shape()
    _refused(_front_end(128, 8192, 8, 160), net, says="65536 steps.*make the two launches")


# 5. more clips than compute units

def test_three_hundred_clips_and_batch_position(oracle_c):
    """300 clips of 5 bins x 4 thresholds, N = 100: rows and stats of every clip against the two launches, rows 0, 255, 256
    and 299 against the oracle, and the same rows from three launches of 100 clips: neither the position in the batch nor the
    workspace slot matters."""
    import torch
    from lsm_speech_classifier_amd import pipeline, synth
    fe, net, _ = _build(oracle_c, 128, 5, 4, 160, 100)
    audio = np.ascontiguousarray(synth.class_chirps(np.arange(300) % 12, seed=77, n_samples=800))
    got = _check(oracle_c, fe, net, audio, oracle_clips=(0, 255, 256, 299))[0]
    x = torch.from_numpy(audio).cuda()
    thirds = torch.cat([pipeline.step_fused(fe, net, x[i:i + 100]) for i in (0, 100, 200)])
    assert torch.equal(thirds, got)
