"""Ring rows in pair blocks for reservoirs with 129 to 256 input channels (csrc/lif_pair.h, INMASK 3: a neuron's inputs as
one (bit position -> row word) entry per coloured bit, held as a position mask and three bit planes and resolved by seven
bitwise selects), and `plan()["ring_form"]` (lsm_reservoir_ring_form).

Reference: the plain-C oracle (oracle/lsm_oracle.c), bit for bit on features, spike matrix, float32 membrane trace and the
in-kernel statistics; one test recomputes the input path in NumPy from the input map alone.  The channel counts: 129 = one
bit in a fifth row word, 160 = exactly five words, 200 = a partly filled seventh word, 256 = eight full words, where the
colouring must be exactly equitable (8 channels per colour)."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE = (129, 160, 200, 256)
N, K, N_OUT, T = 1024, 60, 300, 90


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def pairs_by_default(channels, blocks_per_wave, waves):
    """The rule of choose_pair (csrc/reservoir.hip) for "ring" and auto: pair blocks with at least three blocks per wave up
    to 128 channels; above 128 channels by name only (PAIR_WIDE_AUTO is off: no measured gain over the quads is on record,
    profiles/pair_wide_channels.txt), and in no case by default in the 16-wave layout."""
    return blocks_per_wave >= 3 and channels <= 128 and waves in (4, 8, 16)


# ----------------------------------------------------------------------------- helpers ----
def _rasters(c, t=T, clips=3, bytes_01=False):
    from lsm_speech_classifier_amd import synth
    r = synth.bernoulli_raster(clips, c, t, 0.25, seed=c)
    if not bytes_01:
        r[1] *= 201                                            # any non-zero byte is a spike
    return r


@functools.lru_cache(maxsize=None)
def _built(n, k, n_out, c, t, divisor=None):
    from lsm_speech_classifier_amd import reservoir as R
    from oracle import ref_numpy as O
    wc = O.w_critico(k, 2.0, 2, _rasters(c, t, bytes_01=True))
    kw = {} if divisor is None else {"leak_variance_divisor": divisor}
    return R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                mean_weight=wc * 0.6, **kw), c)


def _set_input_map(res, in_tgt):
    c, fan = in_tgt.shape
    n = res.num_neurons
    flat_c, flat_i = np.repeat(np.arange(c, dtype=np.int32), fan), in_tgt.reshape(-1)
    o2 = np.lexsort((flat_c, flat_i))
    in_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(flat_i, minlength=n), out=in_ptr[1:])
    res.n_channels, res.in_fanout, res.in_tgt = c, fan, np.ascontiguousarray(in_tgt, dtype=np.int32)
    res.in_ptr, res.in_chan = in_ptr, flat_c[o2].astype(np.int32)


def _hub_map(n, c, hub_channels, fan=5):
    """The first `hub_channels` channels all feed neuron 0; every (channel, neuron) pair occurs once."""
    rs = np.random.RandomState(hub_channels)
    in_tgt = np.empty((c, fan), dtype=np.int32)
    for ch in range(c):
        others = rs.choice(np.arange(1, n), fan - 1, replace=False)
        first = 0 if ch < hub_channels else int(rs.randint(1, n))
        while first in others:
            first = int(rs.randint(1, n))
        in_tgt[ch] = np.sort(np.append(others, first))
    return in_tgt


def _oracle(oracle_c, res, rasters):
    out = []
    for r in rasters:
        f, sm, vt = oracle_c.lif_run(res, r, None, want_trace=True)
        per = sm.sum(axis=0, dtype=np.int64)
        out.append((f, sm, vt, [int(np.count_nonzero(per)), int(per.sum())]))
    return out


def _assert_run_equals(net, rasters, ref, wpc, msg):
    import torch
    stats = torch.full((len(rasters), 2), -1, dtype=torch.int32, device="cuda")
    f, sm, vt = net.run_batch(rasters, None, want_spike_matrix=True, want_v_trace=True, waves_per_clip=wpc, stats_out=stats)
    f, sm, vt, stats = f.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy(), stats.cpu().numpy()
    for b, (f_ref, sm_ref, vt_ref, st_ref) in enumerate(ref):
        np.testing.assert_array_equal(sm[b], sm_ref, err_msg=f"spike matrix, clip {b}, {msg}, waves_per_clip {wpc}")
        np.testing.assert_array_equal(vt[b], vt_ref, err_msg=f"membrane trace, clip {b}, {msg}, waves_per_clip {wpc}")
        np.testing.assert_array_equal(f[b], f_ref, err_msg=f"features, clip {b}, {msg}, waves_per_clip {wpc}")
        assert stats[b].tolist() == st_ref, f"statistics, clip {b}, {msg}, waves_per_clip {wpc}"


# ------------------------------------------------------------------------ parity by name ----
@pytest.mark.parametrize("c", WIDE)
def test_pair_blocks_by_name_match_the_oracle(torch_cuda, oracle_c, c):
    from lsm_speech_classifier_amd import snn
    res = _built(N, K, N_OUT, c, T)
    rasters = _rasters(c)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")                               # refused above 128 channels before this form existed
    ref = _oracle(oracle_c, res, rasters)
    assert all(r[3][1] > 100 for r in ref)                     # the reservoir does spike
    for wpc in (0, 4):
        plan = net.plan(3, T, wpc)
        assert plan["kernel"] == "ring" and plan["ring_form"] == "pairs" and plan["input_mode"] == 11, plan
        assert plan["waves_per_clip"] == 4 and plan["slots_per_lane"] == 4
        _assert_run_equals(net, rasters, ref, wpc, "ring-pairs")
    net.set_kernel("ring-quads")
    assert net.plan(3, T, 4)["ring_form"] == "quads" and net.plan(3, T, 4)["input_mode"] in (10, 11)
    _assert_run_equals(net, rasters, ref, 4, "ring-quads")
    net.set_kernel("dense")
    assert net.plan(3, T, 0)["ring_form"] is None
    _assert_run_equals(net, rasters, ref, 0, "dense")


# -------------------------------------------------------------------------- row extremes ----
def _extreme_rasters(c, t):
    r = np.zeros((3, c, t), dtype=np.uint8)
    r[1] = 1                                                   # every entry counted on every step: the count is the fan-in
    r[2, np.arange(t) % c, np.arange(t)] = 1                   # one channel per step
    return r


def test_row_extremes_at_256_channels(torch_cuda, oracle_c):
    from lsm_speech_classifier_amd import snn
    c, t = 256, 270                                            # every channel gets its step
    res = _built(N, K, N_OUT, c, T)
    rasters = _extreme_rasters(c, t)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")
    ref = _oracle(oracle_c, res, rasters)
    assert ref[0][3] == [0, 0] and ref[1][3][1] > 1000
    for wpc in (4, 8):
        assert net.plan(3, t, wpc)["input_mode"] == 11
        _assert_run_equals(net, rasters, ref, wpc, "ring-pairs, row extremes")


def test_input_path_recomputed_from_the_input_map(torch_cuda):
    """No recurrent weights and a threshold above reach: the membrane trace is v <- (v - leak * v) + w_in * count in
    float32 (SPEC.md 3), with the count taken here from in_tgt alone.  One channel spikes per step, so a wrong word
    index or position for any single (channel, neuron) entry changes the trace."""
    from lsm_speech_classifier_amd import snn
    c, t = 256, 270
    res = copy.copy(_built(N, K, N_OUT, c, T))
    res.csc_w, res.csr_w = np.zeros_like(res.csc_w), np.zeros_like(res.csr_w)
    res.theta = np.float32(1e30)
    raster = _extreme_rasters(c, t)[2:]
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")
    assert net.plan(1, t, 4)["input_mode"] == 11
    _, sm, vt = net.run_batch(raster, None, want_spike_matrix=True, want_v_trace=True, waves_per_clip=4)
    assert not sm.any().item()
    v = np.zeros(N, dtype=np.float32)
    leak, w_in = res.leak.astype(np.float32), np.float32(res.w_in)
    want = np.empty((t, N), dtype=np.float32)
    for step in range(t):
        count = np.zeros(N, dtype=np.float32)
        np.add.at(count, res.in_tgt[step % c], np.float32(1))
        v = (v - leak * v) + (np.float32(0) + w_in * count)
        want[step] = v
    assert len(np.unique(want[-1])) > 3
    np.testing.assert_array_equal(vt[0].cpu().numpy(), want)


# ---------------------------------------------------------------------- per-neuron leaks ----
def test_per_neuron_leaks_with_four_blocks_per_wave(torch_cuda, oracle_c):
    """leak_variance_divisor: a leak coefficient per neuron in registers next to the bit planes, 8 neurons per lane at 8
    waves (the kernel form with the most registers) and 4 per lane at 16."""
    from lsm_speech_classifier_amd import snn
    n, k, c, t = 4096, 300, 256, 60
    res = _built(n, k, n // 3, c, t, 5.0)
    assert len(np.unique(res.leak)) > 100
    rasters = _rasters(c, t, clips=2)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")
    ref = _oracle(oracle_c, res, rasters)
    assert all(r[3][1] > 100 for r in ref)
    for wpc, slots in ((8, 8), (16, 4)):
        plan = net.plan(2, t, wpc)
        assert (plan["ring_form"], plan["input_mode"], plan["slots_per_lane"]) == ("pairs", 11, slots), plan
        _assert_run_equals(net, rasters, ref, wpc, "ring-pairs, per-neuron leaks")
    # auto serves this reservoir with ring rows (64 MB of dense rows): the same rule as "ring"
    net.set_kernel("auto")
    plan = net.plan(2, t, 0)
    assert plan["kernel"] == "ring" and plan["ring_form"] == ("pairs" if pairs_by_default(c, 4, 8) else "quads"), plan


# -------------------------------------------------------------------------- auto's choice ----
def test_what_ring_takes_above_128_channels(torch_cuda, oracle_c):
    from lsm_speech_classifier_amd import snn
    n, k, c, t = 1536, 300, 200, 60                            # 12 blocks: three per wave at 4 waves
    res = _built(n, k, n // 3, c, t)
    rasters = _rasters(c, t, clips=2)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")
    assert (net.plan(2, t, 0)["waves_per_clip"], net.plan(2, t, 0)["slots_per_lane"]) == (4, 6)
    net.set_kernel("ring")
    plan = net.plan(2, t, 0)
    if pairs_by_default(c, 3, 4):
        assert plan["ring_form"] == "pairs" and plan["input_mode"] == 11, plan
    else:
        # quads in whichever ownership "ring-quads" takes here (6 quads: no strided layout, contiguous ownership)
        net.set_kernel("ring-quads")
        assert plan == net.plan(2, t, 0) and plan["ring_form"] in ("quads", "quads-contiguous"), plan
        assert plan["input_mode"] in (10, 11)
        net.set_kernel("ring")
    _assert_run_equals(net, rasters, _oracle(oracle_c, res, rasters), 0, "ring")
    net.set_kernel("auto")                                     # 9 MB of dense rows: auto stays dense here
    assert net.plan(2, t, 0)["ring_form"] is None


def test_no_pair_blocks_by_default_where_the_layout_needs_16_waves(torch_cuda):
    """N = 8192 with a window of more than 8 blocks (BASELINE configs[4]'s class: N = 8000, k = 1600, 256 filters): the
    pair layout has 16 waves.  "ring" and auto plan quads; pair blocks by name only.  Plans alone, no launch."""
    from lsm_speech_classifier_amd import reservoir as R, snn
    res = R.build_reservoir(R.SimulationParams(num_neurons=8192, num_output_neurons=64, small_world_graph_k=1640,
                                               mean_weight=0.001), 256)
    net = snn.SNN(None, reservoir=res)
    assert not pairs_by_default(256, 4, 16)
    for kernel in ("auto", "ring"):
        net.set_kernel(kernel)
        for wpc in (0, 16):
            plan = net.plan(1024, 400, wpc)
            assert plan["kernel"] == "ring" and plan["ring_form"] == "quads" and plan["input_mode"] in (10, 11), (kernel, plan)
    net.set_kernel("ring-pairs")
    plan = net.plan(1024, 400, 0)
    assert (plan["ring_form"], plan["waves_per_clip"], plan["slots_per_lane"], plan["input_mode"]) == ("pairs", 16, 8, 11)


# ------------------------------------------------------------------------------ refusals ----
@pytest.mark.parametrize("case", ["257 channels", "33 channels onto one neuron"])
def test_maps_without_a_pair_form_run_in_quads(torch_cuda, oracle_c, case):
    from lsm_speech_classifier_amd import _lib, snn
    if case == "257 channels":
        c = 257
        res = _built(N, K, N_OUT, c, T)
    else:
        c = 160
        res = copy.copy(_built(N, K, N_OUT, c, T))
        _set_input_map(res, _hub_map(N, c, 33))
    rasters = _rasters(c)
    net = snn.SNN(None, reservoir=res)
    with pytest.raises(_lib.LsmHipError, match="pair-block"):
        net.set_kernel("ring-pairs")
    net.set_kernel("ring")
    ref = _oracle(oracle_c, res, rasters)
    for wpc in (0, 4):
        plan = net.plan(3, T, wpc)
        assert plan["ring_form"] in ("quads", "quads-contiguous") and plan["input_mode"] in (10, 11), plan
        _assert_run_equals(net, rasters, ref, wpc, f"ring, {case}")


def test_32_channels_onto_one_neuron_still_have_pair_blocks(torch_cuda, oracle_c):
    from lsm_speech_classifier_amd import snn
    c = 160
    res = copy.copy(_built(N, K, N_OUT, c, T))
    _set_input_map(res, _hub_map(N, c, 32))
    rasters = _rasters(c)
    rasters[2, :32] = 1                                        # all 32 of neuron 0's channels at once
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("ring-pairs")
    assert net.plan(3, T, 4)["input_mode"] == 11
    ref = _oracle(oracle_c, res, rasters)
    for wpc in (4, 8):
        _assert_run_equals(net, rasters, ref, wpc, "ring-pairs, 32-channel hub")


# --------------------------------------------------------------- ring_form on the old ground ----
def test_ring_form_of_the_existing_kernels(torch_cuda):
    from lsm_speech_classifier_amd import reservoir as R, snn
    net = snn.SNN(None, reservoir=_built(N, K, N_OUT, 96, T))
    for kernel, form in (("dense", None), ("sparse", None), ("ring-contiguous", "quads-contiguous"), ("ring-quads", "quads"),
                         ("ring-pairs", "pairs")):
        net.set_kernel(kernel)
        assert net.plan(3, T, 4)["ring_form"] == form, kernel
    # BASELINE configs[3]: N = 4000, k = 800, 128 filters -- auto plans pair blocks, 8 waves of four blocks
    res = R.build_reservoir(R.SimulationParams(num_neurons=4000, num_output_neurons=1600, small_world_graph_k=800,
                                               mean_weight=0.001), 128)
    plan = snn.SNN(None, reservoir=res).plan(1024, 400, 0)
    assert (plan["kernel"], plan["ring_form"], plan["waves_per_clip"], plan["input_mode"]) == ("ring", "pairs", 8, 15), plan
