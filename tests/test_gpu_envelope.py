"""The reservoir kernels over the whole range the C ABI accepts (include/lsm_hip.h, SPEC.md 4): n_steps and n_channels
up to 65535, any refractory period >= 0, any burst limit, any input map whose targets are in range.  The other GPU
tests stay near the reference's operating point (T <= 400, C <= 256, refractory 0-5, burst limit 4 or 5, input maps
drawn without replacement); the kernels pack their state into narrow fields whose limits those shapes never reach:

  * the feature record {n | bursts << 16, first | last << 16, sum t, sum isi^2} of every kernel,
  * (output slot + 1) | (refractory countdown << 16) in one register of the ring and pair kernels,
  * c >> 5 in 11 bits and 16-bit input counts in the ring kernel's input entries,
  * the per-clip LDS plan of every kernel against a CU's 160 KB, and the sparse kernel's SEGLDS switch on T.

Reference: the plain-C oracle (oracle/lsm_oracle.c: int32 / int64 accumulators), bit for bit on features, spike
matrix, float32 membrane trace and the in-kernel statistics; for the long clips a second, formula-free reference in
float64 NumPy computed from the spike matrix."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
INTEGER_KEYS = ('spike_counts', 'first_spike_times', 'last_spike_times', 'burst_counts')
KERNELS = ("dense", "sparse", "ring-pairs", "ring-quads", "ring-contiguous")
ENTRY_MODES = (0, 1, 10, 11, 20)                    # input drive from input-map entries (lsm_reservoir_input_mode)
MASK_MODES = (2, 3, 12, 13, 14, 15)                 # ... from per-neuron channel masks
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


# ----------------------------------------------------------------------------- helpers ----
@functools.lru_cache(maxsize=None)
def _built(n, k, n_out, c, mean_weight, refractory=2):
    from lsm_speech_classifier_amd import reservoir as R
    return R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                mean_weight=mean_weight, refractory_period=refractory), c)


def _reservoir(n, k, n_out, c, mean_weight, **fields):
    """A reservoir as the builder makes it, then a shallow copy with some fields overwritten (the same object
    goes to the library and to the oracle)."""
    res = copy.copy(_built(n, k, n_out, c, mean_weight))
    for name, value in fields.items():
        assert hasattr(res, name), name
        setattr(res, name, value)
    return res


def _set_input_map(res, in_tgt):
    """Overwrite the input map of `res`: (C, fan-out) targets per channel plus the by-neuron view the oracle reads."""
    c, fan = in_tgt.shape
    n = res.num_neurons
    flat_c, flat_i = np.repeat(np.arange(c, dtype=np.int32), fan), in_tgt.reshape(-1)
    o2 = np.lexsort((flat_c, flat_i))
    in_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(flat_i, minlength=n), out=in_ptr[1:])
    res.in_fanout, res.in_tgt, res.in_ptr, res.in_chan = fan, in_tgt, in_ptr, flat_c[o2].astype(np.int32)


def _offered(net):
    """The kernel families (`SNN.set_kernel` names) this reservoir offers."""
    from lsm_speech_classifier_amd import _lib
    out = []
    for kernel in KERNELS:
        try:
            net.set_kernel(kernel)
            out.append(kernel)
        except _lib.LsmHipError:
            pass
    net.set_kernel("auto")
    return out


def _oracle(oracle_c, res, rasters, keys=None, want_trace=True):
    """Per clip (features, spike matrix, trace or None, [neurons that fired, spikes]) from the C oracle."""
    out = []
    for r in rasters:
        f, sm, vt = oracle_c.lif_run(res, r, keys, want_trace=want_trace)
        per = sm.sum(axis=0, dtype=np.int64)
        out.append((f, sm, vt, [int(np.count_nonzero(per)), int(per.sum())]))
    return out


def _run(net, rasters, wpc, keys=None, want_trace=True):
    """One launch; None when a FORCED layout does not exist for this reservoir (a "layout" error), else
    (features, spike matrix, trace or None, statistics) as NumPy arrays."""
    import torch
    from lsm_speech_classifier_amd import _lib
    stats = torch.full((len(rasters), 2), -1, dtype=torch.int32, device="cuda")
    try:
        f, sm, vt = net.run_batch(rasters, keys, want_spike_matrix=True, want_v_trace=want_trace,
                                  waves_per_clip=wpc, stats_out=stats)
    except _lib.LsmHipError as e:
        if wpc != 0 and "layout" in str(e):
            return None
        raise
    return f.cpu().numpy(), sm.cpu().numpy(), (vt.cpu().numpy() if want_trace else None), stats.cpu().numpy()


def _assert_equal(got, ref, msg):
    f, sm, vt, stats = got
    for b, (f_ref, sm_ref, vt_ref, st_ref) in enumerate(ref):
        np.testing.assert_array_equal(sm[b], sm_ref, err_msg=f"spike matrix, clip {b}, {msg}")
        if vt is not None:
            np.testing.assert_array_equal(vt[b], vt_ref, err_msg=f"membrane trace, clip {b}, {msg}")
        np.testing.assert_array_equal(f[b], f_ref, err_msg=f"features, clip {b}, {msg}")
        assert stats[b].tolist() == st_ref, f"statistics, clip {b}, {msg}"


def _check(net, res, rasters, oracle_c, kernels, forced, keys=None, want_trace=True, ref=None):
    """Every kernel in `kernels` with the library's own layout (waves_per_clip = 0) and the forced one(s) against the
    oracle.  Returns the oracle's results and the number of launches compared."""
    if ref is None:
        ref = _oracle(oracle_c, res, rasters, keys, want_trace)
    offered = _offered(net)
    ran = 0
    for kernel in kernels:
        assert kernel in offered, f"{kernel} is not offered for N={res.num_neurons}, C={res.n_channels}: {offered}"
        net.set_kernel(kernel)
        for wpc in (0,) + tuple(forced.get(kernel, ())):
            got = _run(net, rasters, wpc, keys, want_trace)
            if got is None:
                continue
            _assert_equal(got, ref, f"kernel {kernel}, waves_per_clip {wpc}")
            ran += 1
    net.set_kernel("auto")
    return ref, ran


# ------------------------------------------------- 1. long clips and the 16-bit feature fields ----
def _crafted_raster(c, t, seed):
    """Channel 0 on at every step, 1 at steps 0 and T-1 only, 2 at the last three steps only, 3 at every 257th
    step, the others Bernoulli(0.01).  With theta = 2.0, w_in = 2.5 and no refractory period every active channel
    fires its targets at once: counts up to T, first spikes up to T-3, one interval of T-1, T-1 bursts."""
    r = (np.random.default_rng(seed).random((c, t)) < 0.01).astype(np.uint8)
    r[0] = 1
    r[1] = 0
    r[1, [0, t - 1]] = 1
    r[2] = 0
    r[2, t - 3:] = 1
    r[3] = 0
    r[3, ::257] = 1
    return r


def _long_clip_case(n, t):
    # recurrent weights so weak that activity does not spread: the spike trains are the crafted input's
    k, n_out, mean_weight = (20, 130, 0.002) if n == 130 else (24, 64, 0.02)
    res = _reservoir(n, k, n_out, 24, mean_weight, theta=np.float32(2.0), w_in=np.float32(2.5), refractory_period=0)
    rasters = np.zeros((2, 24, t), dtype=np.uint8)
    rasters[0] = _crafted_raster(24, t, seed=t)              # clip 1 stays silent: neighbour independence
    # Channels 1 and 2 must each be the ONLY input of one output neuron, or no neuron shows their spike train alone.
    # The builder's map gives that at N = 1024; at N = 130 (fan-out 5) every target of channel 2 is shared with a
    # Bernoulli channel: those channels (two or three of the twenty) stay silent.
    for ch in (1, 2):
        for i in res.in_tgt[ch]:
            rivals = set(res.in_chan[res.in_ptr[i]:res.in_ptr[i + 1]].tolist()) - {ch}
            if i in res.out_idx and not rivals & {0, 1, 2, 3}:
                rasters[0, sorted(rivals)] = 0
                break
        else:
            raise AssertionError(f"channel {ch} has no output target of its own")
    assert rasters[0, 4:].any(axis=1).sum() >= 15
    return res, rasters


def _assert_input_reaches_the_field_limits(res, f_ref, t):
    f = dict(zip(ALL_KEYS, f_ref.reshape(8, len(res.out_idx))))
    assert f['spike_counts'].max() == t
    assert f['first_spike_times'].max() == t - 3
    assert f['last_spike_times'].max() == t - 1
    assert f['mean_isi'].max() == t - 1                       # two spikes, at 0 and T-1
    assert f['burst_counts'].max() == t - 1
    if t >= 33000:
        assert t - 3 >= 32768 and f['mean_isi'].max() > 32767


def _features_from_definition(sm, out_idx, t, burst_isi_max):
    """SPEC.md 4 straight from the (T, N) spike matrix, float64, no one-pass formulas; undefined entries 0."""
    out = {k: np.zeros(len(out_idx)) for k in ALL_KEYS}
    for o, i in enumerate(out_idx):
        col = sm[:, i].astype(np.float64)
        times = np.nonzero(sm[:, i])[0].astype(np.float64)
        out['spike_counts'][o] = len(times)
        out['spike_variances'][o] = np.var(col)
        if len(times) >= 1:
            out['mean_spike_times'][o] = times.mean()
            out['first_spike_times'][o] = times[0]
            out['last_spike_times'][o] = times[-1]
        if len(times) >= 2:
            isi = np.diff(times)
            out['mean_isi'][o] = isi.mean()
            out['isi_variances'][o] = np.var(isi)
            out['burst_counts'][o] = (isi <= burst_isi_max).sum()
    return out


def _assert_features_follow_the_definition(f_gpu, sm_gpu, res, t, msg):
    """|gpu - float32(ref)| <= 2^-23 |ref| + 2^-50 T^2: one float32 rounding of the result, plus the cancellation in
    Q/(n-1) - m^2, evaluated in float64 (2^-53 relative) on operands up to T^2; integer-valued features are equal."""
    ref = _features_from_definition(sm_gpu, res.out_idx, t, res.burst_isi_max)
    got = dict(zip(ALL_KEYS, f_gpu.reshape(8, len(res.out_idx)).astype(np.float64)))
    for key in ALL_KEYS:
        if key in INTEGER_KEYS:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{key}, {msg}")
        else:
            err = np.abs(got[key] - ref[key].astype(np.float32).astype(np.float64))
            bound = 2.0 ** -23 * np.abs(ref[key]) + 2.0 ** -50 * t * t
            assert (err <= bound).all(), f"{key}, {msg}: error {err.max()} beyond {bound[np.argmax(err - bound)]}"


@pytest.mark.parametrize("t", [401, 1023, 4099, 33000])
def test_long_clips_small_reservoir(torch_cuda, oracle_c, t):
    """N = 130, dense and sparse kernel.  waves_per_clip = 1 puts all 130 neurons into one wave (four per lane)."""
    from lsm_speech_classifier_amd import snn
    res, rasters = _long_clip_case(130, t)
    ref = _oracle(oracle_c, res, rasters, ALL_KEYS)
    _assert_input_reaches_the_field_limits(res, ref[0][0], t)
    assert ref[1][3] == [0, 0]
    net = snn.SNN(None, reservoir=res)
    _, ran = _check(net, res, rasters, oracle_c, ("dense", "sparse"), {"dense": (1,), "sparse": (1,)}, ALL_KEYS, ref=ref)
    assert ran == 4                                           # a reservoir of 130 neurons has the one-wave layout
    if t <= 4099:
        for kernel in ("dense", "sparse"):
            net.set_kernel(kernel)
            f, sm, _, _ = _run(net, rasters, 0, ALL_KEYS, want_trace=False)
            _assert_features_follow_the_definition(f[0], sm[0], res, t, f"kernel {kernel}")


@pytest.mark.parametrize("t", [4099, 33000])
def test_long_clips_all_kernels(torch_cuda, oracle_c, t):
    """N = 1024, all five kernels; features, statistics and spike matrix (the trace would be 135 MB per clip).
    The dense kernel keeps the feature records in registers up to four neurons per lane and in LDS beyond: at
    N = 1024 waves_per_clip = 1 and 2 give 16 and 8 neurons per lane (the LDS records), the library's own choice 1."""
    from lsm_speech_classifier_amd import snn
    res, rasters = _long_clip_case(1024, t)
    ref = _oracle(oracle_c, res, rasters, ALL_KEYS, want_trace=False)
    _assert_input_reaches_the_field_limits(res, ref[0][0], t)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("dense")
    assert net.plan(2, t, 1)["slots_per_lane"] == 16 and net.plan(2, t, 0)["slots_per_lane"] <= 4
    forced = {"dense": (1, 2), "sparse": (1,), "ring-pairs": (4,), "ring-quads": (4,), "ring-contiguous": (4,)}
    _, ran = _check(net, res, rasters, oracle_c, KERNELS, forced, ALL_KEYS, want_trace=False, ref=ref)
    assert ran >= 5 + 3                                       # the dense and sparse layouts above exist for every N <= 1024
    if t <= 4099:
        for kernel in KERNELS:
            net.set_kernel(kernel)
            f, sm, _, _ = _run(net, rasters, 0, ALL_KEYS, want_trace=False)
            _assert_features_follow_the_definition(f[0], sm[0], res, t, f"kernel {kernel}")


# ------------------------------------------------------------ 2. the last T a plan accepts ----
def _last_accepted_steps(net):
    """Largest n_steps in [1, 65535] that plan(1, n_steps, 0) accepts (the LDS image grows with n_steps)."""
    from lsm_speech_classifier_amd import _lib

    def accepted(t):
        try:
            net.plan(1, t, 0)
            return True
        except _lib.LsmHipError as e:
            assert "layout" in str(e), str(e)
            return False
    lo, hi = 1, 65536                                         # accepted(lo), not accepted(hi)
    assert accepted(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepted(mid):
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("kernel", KERNELS)
def test_last_step_count_a_plan_accepts(torch_cuda, oracle_c, kernel):
    """At the largest n_steps a kernel family accepts its LDS image is at most a CU's 160 KB and the run equals the
    oracle (an under-counted LDS formula would corrupt the input bits of the last steps); one step more is refused
    by plan and run with a message, and the handle still works afterwards."""
    from lsm_speech_classifier_amd import _lib, snn, synth
    n, k, n_out, c = (192, 30, 64, 256) if kernel in ("dense", "sparse") else (1024, 24, 64, 128)
    res = _reservoir(n, k, n_out, c, 0.05)
    net = snn.SNN(None, reservoir=res)
    assert kernel in _offered(net)
    net.set_kernel(kernel)
    t_max = _last_accepted_steps(net)
    assert 1000 < t_max < 65535, t_max                        # the LDS bounds it, not the ABI's 65535
    plan = net.plan(1, t_max, 0)
    assert plan["kernel"] == ("ring" if kernel.startswith("ring") else kernel)
    assert plan["lds_bytes"] <= LDS_PER_CU
    # the image grows by the input bits of one step, 4 * ceil(C / 32) bytes: the last T is the last that fits
    assert plan["lds_bytes"] + 4 * ((c + 31) // 32) > LDS_PER_CU
    rasters = synth.bernoulli_raster(1, c, t_max + 1, 0.2, seed=n)
    ref = _oracle(oracle_c, res, rasters[:, :, :t_max], ALL_KEYS, want_trace=False)
    assert ref[0][3][1] > t_max                               # the reservoir spikes
    assert ref[0][1][-8:].any()                               # ... in the last steps too
    _assert_equal(_run(net, np.ascontiguousarray(rasters[:, :, :t_max]), 0, ALL_KEYS, want_trace=False), ref,
                  f"kernel {kernel}, T = {t_max}")
    with pytest.raises(_lib.LsmHipError, match="layout"):
        net.plan(1, t_max + 1, 0)
    with pytest.raises(_lib.LsmHipError, match="layout"):
        net.run_batch(rasters, ALL_KEYS)
    small = np.ascontiguousarray(rasters[:, :, :50])
    _assert_equal(_run(net, small, 0, ALL_KEYS), _oracle(oracle_c, res, small, ALL_KEYS), f"kernel {kernel} after a refusal")
    with pytest.raises(_lib.LsmHipError, match="bad n_clips/n_steps"):
        net.run_batch(np.zeros((1, c, 65536), dtype=np.uint8), ALL_KEYS)
    with pytest.raises(_lib.LsmHipError, match="bad n_clips/n_steps"):
        net.plan(1, 65536, 0)


def test_sparse_kernel_on_both_sides_of_the_segment_table_switch(torch_cuda, oracle_c):
    """The sparse kernel stages its segment table in LDS (SEGLDS) while core + table <= 80 KB (csrc/reservoir.hip:
    lif_lds_core, lif_seg_bytes, lif_seg_in_lds); the flip point in T is computed here from those formulas and
    checked against plan's lds_bytes, then one T on each side runs against the oracle."""
    from lsm_speech_classifier_amd import snn, synth
    n, k, n_out, c, wpc = 192, 30, 64, 256, 4
    res = _reservoir(n, k, n_out, c, 0.05)
    net = snn.SNN(None, reservoir=res)
    net.set_kernel("sparse")
    p = net.plan(1, 400, wpc)
    assert p["kernel"] == "sparse" and p["waves_per_clip"] == wpc
    npad, cw = p["slots_per_lane"] * 64 * wpc, (c + 31) // 32

    def core(t):
        return npad * 4 + npad * 4 + 2 * npad * 2 + 128 + n_out * 16 + t * cw * 4
    seg = (n + 1) * 4 + ((n * (wpc + 1) + 1) // 2) * 4
    t_in = (80 * 1024 - seg - core(0)) // (cw * 4)            # the last T with the table in LDS
    assert core(t_in) + seg <= 80 * 1024 < core(t_in + 1) + seg and t_in > 400
    assert net.plan(1, t_in, wpc)["lds_bytes"] == core(t_in) + seg
    assert net.plan(1, t_in + 1, wpc)["lds_bytes"] == core(t_in + 1)
    rasters = synth.bernoulli_raster(2, c, t_in + 1, 0.2, seed=5)
    for t in (t_in, t_in + 1):
        r = np.ascontiguousarray(rasters[:, :, :t])
        ref = _oracle(oracle_c, res, r, ALL_KEYS)
        assert ref[0][3][1] > t
        for w in (wpc, 0):
            assert net.plan(2, t, w)["kernel"] == "sparse"
            _assert_equal(_run(net, r, w, ALL_KEYS), ref, f"sparse, T = {t}, waves_per_clip {w}")


# ----------------------------------------------- 3. refractory periods beyond the tested 0..5 ----
REFRACTORY = [7, 64, 399, 400, 65535, 65536, 65537, 100000]
FORCED_1024 = {"dense": (2,), "sparse": (1,), "ring-pairs": (8,), "ring-quads": (2,), "ring-contiguous": (4,)}
FORCED_130 = {"dense": (1,), "sparse": (2,)}


def _mid_case(n=1024):
    from lsm_speech_classifier_amd import synth
    k, n_out = (24, 64) if n == 1024 else (20, 130)
    return (n, k, n_out, 24, 0.05), synth.bernoulli_raster(2, 24, 400, 0.3, seed=n)


@pytest.mark.parametrize("refractory", REFRACTORY)
def test_refractory_periods_all_kernels(torch_cuda, oracle_c, refractory):
    """N = 1024, T = 400.  The ring and pair kernels keep the countdown in the upper 16 bits of a register; the
    dense and sparse kernels and the oracle in an int.  A period of T - 1 or more holds a neuron that fired to the
    end of the clip, whatever its value."""
    from lsm_speech_classifier_amd import snn
    shape, rasters = _mid_case(1024)
    res = _reservoir(*shape, refractory_period=refractory)
    net = snn.SNN(None, reservoir=res)
    ref, ran = _check(net, res, rasters, oracle_c, KERNELS, FORCED_1024, ALL_KEYS)
    assert ran >= 5
    total = sum(r[3][1] for r in ref)
    assert total > 0
    if refractory >= 399:
        for f_ref, sm_ref, _, _ in ref:
            assert sm_ref.sum(axis=0).max() == 1
            assert f_ref[:len(res.out_idx)].max() <= 1        # spike_counts


@pytest.mark.parametrize("refractory", [2] + REFRACTORY)
def test_refractory_periods_small_reservoir(torch_cuda, oracle_c, refractory):
    """N = 130, dense and sparse: the dense kernel counts a period of 2 (the reference's) down in scalar lane masks
    (REFM) and every other period in vector registers."""
    from lsm_speech_classifier_amd import snn
    shape, rasters = _mid_case(130)
    res = _reservoir(*shape, refractory_period=refractory)
    net = snn.SNN(None, reservoir=res)
    ref, ran = _check(net, res, rasters, oracle_c, ("dense", "sparse"), FORCED_130, ALL_KEYS)
    assert ran == 4
    assert sum(r[3][1] for r in ref) > 0
    if refractory >= 399:
        assert max(r[1].sum(axis=0).max() for r in ref) == 1


# ------------------------------------------------------------------------- 4. burst limit ----
@pytest.mark.parametrize("burst_isi_max", [-1, 0, 1, 399, 70000])
def test_burst_limits_all_kernels(torch_cuda, oracle_c, burst_isi_max):
    """Any int is a burst limit: none or a negative one counts no interval, one of T - 1 or more counts all."""
    from lsm_speech_classifier_amd import snn
    shape, rasters = _mid_case(1024)
    res = _reservoir(*shape, burst_isi_max=burst_isi_max)
    net = snn.SNN(None, reservoir=res)
    ref, ran = _check(net, res, rasters, oracle_c, KERNELS, FORCED_1024, ALL_KEYS)
    assert ran >= 5
    n_out = len(res.out_idx)
    for f_ref, _, _, _ in ref:
        counts, bursts = f_ref[:n_out], f_ref[7 * n_out:]
        assert counts.max() >= 2                              # there are intervals to count
        if burst_isi_max <= 0:
            assert not bursts.any()
        elif burst_isi_max >= 399:
            np.testing.assert_array_equal(bursts, np.maximum(counts - 1, 0))


# ------------------------------------------------------------------ 5. many input channels ----
@pytest.mark.parametrize("n,c,t", [(1000, 1000, 60), (300, 4097, 24), (2048, 2000, 40), (64, 65535, 8)])
def test_many_input_channels(torch_cuda, oracle_c, n, c, t):
    """Input maps far beyond the 128 channels of the mask modes: entry lists of thousands per wave, 16-bit counts
    (64 neurons fed by 65535 channels: about a thousand channels per neuron), c >> 5 up to 2047."""
    from lsm_speech_classifier_amd import snn, synth
    res = _reservoir(n, 24, n // 2, c, 0.05)
    rasters = synth.bernoulli_raster(2, c, t, 0.3, seed=c)
    net = snn.SNN(None, reservoir=res)
    offered = _offered(net)
    assert "dense" in offered and "sparse" in offered and "ring-pairs" not in offered     # pair blocks: C <= 128
    if n == 2048:
        assert "ring-quads" in offered and "ring-contiguous" in offered
    for kernel in offered:
        net.set_kernel(kernel)
        assert net.plan(2, t, 0)["input_mode"] in ENTRY_MODES
    ref, ran = _check(net, res, rasters, oracle_c, offered, {kernel: (4,) for kernel in offered}, ALL_KEYS)
    assert ran >= len(offered)
    assert all(r[3][1] > 0 for r in ref)
    if c == 65535:
        assert np.diff(res.in_ptr).max() > 1000


def test_channel_count_limit_is_enforced_at_create_time(torch_cuda):
    from lsm_speech_classifier_amd import _lib, snn
    res = _reservoir(64, 24, 32, 65535, 0.05)                 # one channel more than the largest accepted map
    res.n_channels, res.in_tgt = 65536, np.vstack([res.in_tgt, res.in_tgt[:1]])
    with pytest.raises(_lib.LsmHipError, match="n_channels=65536"):
        snn.SNN(None, reservoir=res)


# ------------------------------------------- 6. a channel that names the same neuron twice ----
def test_a_channel_that_names_a_neuron_twice_counts_twice(torch_cuda, oracle_c):
    """The oracle adds w_in once per (channel, target) ENTRY of the input map.  Channel masks hold one bit per
    (channel, neuron) pair, so the library must leave the mask modes for such a map: the dense kernel and the ring
    quads fall back to the entry lists.  The pair-block kernel has no entry form (csrc/lif_pair.h counts from masks
    only): asked for by name it is refused with a message, and "ring" serves the reservoir with quads."""
    from lsm_speech_classifier_amd import _lib, snn, synth
    n, k, c, t, fan = 1000, 60, 96, 150, 5
    rasters = synth.bernoulli_raster(2, c, t, 0.3, seed=6)
    res = _reservoir(n, k, 300, c, 0.05)
    rs = np.random.RandomState(6)
    in_tgt = np.stack([np.sort(rs.choice(n, fan, replace=False)) for _ in range(c)]).astype(np.int32)
    _set_input_map(res, in_tgt)                               # fan-out 5, every (channel, neuron) pair once
    clean = snn.SNN(None, reservoir=res)
    assert "ring-pairs" in _offered(clean)                    # with such a map the reservoir has pair blocks
    clean.set_kernel("dense")
    assert clean.plan(2, t, 0)["input_mode"] in MASK_MODES
    in_tgt = in_tgt.copy()
    doubled = np.arange(0, c, 10)[:10]
    in_tgt[doubled, 1] = in_tgt[doubled, 0]                   # ten channels list their first target twice
    twice = copy.copy(res)
    _set_input_map(twice, in_tgt)
    ref = _oracle(oracle_c, twice, rasters, ALL_KEYS)
    ref_clean = _oracle(oracle_c, res, rasters, ALL_KEYS)
    assert not np.array_equal(ref[0][2], ref_clean[0][2])     # the second entry changes the membrane trace
    net = snn.SNN(None, reservoir=twice)
    offered = _offered(net)
    assert "ring-pairs" not in offered
    with pytest.raises(_lib.LsmHipError, match="pair-block"):
        net.set_kernel("ring-pairs")
    kernels = ("dense", "sparse", "ring-quads", "ring-contiguous")
    for kernel in kernels + ("ring",):
        net.set_kernel(kernel)
        for wpc in (0, 4):
            assert net.plan(2, t, wpc)["input_mode"] not in MASK_MODES, (kernel, wpc)
    _, ran = _check(net, twice, rasters, oracle_c, kernels, {kernel: (4,) for kernel in kernels}, ALL_KEYS, ref=ref)
    assert ran == 8
    net.set_kernel("ring")                                    # what the library prefers: quads here
    for wpc in (0, 4, 8):
        got = _run(net, rasters, wpc, ALL_KEYS)
        if got is not None:
            _assert_equal(got, ref, f"kernel ring, waves_per_clip {wpc}")
    assert ref[0][3][1] > 500


# ------------------------------------------------------------------------ 7. repeated keys ----
def test_repeated_feature_keys(torch_cuda, oracle_c):
    from lsm_speech_classifier_amd import _lib, snn
    shape, rasters = _mid_case(130)
    res = _reservoir(*shape)
    net = snn.SNN(None, reservoir=res)
    keys = ["spike_counts", "mean_isi", "spike_counts"]
    ref, ran = _check(net, res, rasters, oracle_c, ("dense", "sparse"), {}, keys)
    assert ran == 2 and ref[0][0].shape == (3 * 130,)
    np.testing.assert_array_equal(ref[0][0][:130], ref[0][0][260:])
    assert ref[0][0][:130].max() >= 2
    with pytest.raises(_lib.LsmHipError, match="n_keys"):
        net.run_batch(rasters, ALL_KEYS + ["spike_counts"])
