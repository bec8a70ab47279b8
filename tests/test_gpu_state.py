"""Reservoir runs that continue from a saved state (SPEC.md 4a, `lsm_reservoir_run_from`, `SNN.run_batch(state=...)`).

A run cut into launches at any step must give, bit for bit, what the uncut run gives.  The reference is the plain-C
oracle (oracle/lsm_oracle.c) on the WHOLE raster, computed once per reservoir; the code under test is never its own
reference, and nothing here has a tolerance.  Every kernel family a reservoir offers runs (dense, sparse, pair blocks,
quads of both ownerships): the last test of the module fails when one of them never did.

Before anything is compared, the oracle's own output must show that the main cut is a cut through activity: spikes at
the step before it, neurons inside their refractory period, output neurons whose spike trains straddle it with an
interval that counts as a burst and with one that does not (the two branches of the record merge)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
TWO_KEYS = ['burst_counts', 'spike_variances']              # a subset, not in the default order
KERNELS = ("dense", "sparse", "ring-pairs", "ring-quads", "ring-contiguous")
SHAPES = [(256, 50, 100, 40), (1024, 204, 410, 64), (1024, 204, 410, 160), (2048, 408, 820, 128)]   # (N, k, n_out, C)
T, B, DENSITY = 96, 3, 0.35
_RAN = set()                                                # kernel families that ran at least one continued launch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


# ----------------------------------------------------------------------------- helpers ----
def _rasters(shape_index, c):
    return np.stack([(np.random.RandomState(100 * shape_index + b).random_sample((c, T)) < DENSITY).astype(np.uint8)
                     for b in range(B)])


def _refractory_after(sm, t, period):
    """Countdown of every neuron after step t, from the (T, N) spike matrix: max(0, R - (t - t_last))."""
    out = np.zeros(sm.shape[1], dtype=np.int64)
    for i in range(sm.shape[1]):
        fired = np.nonzero(sm[:t + 1, i])[0]
        if len(fired):
            out[i] = max(0, period - (t - int(fired[-1])))
    return out


def _cut_is_through_activity(sm, res, ts):
    """The four conditions of the module docstring for a cut before step `ts`, on one clip's oracle spike matrix."""
    if not sm[ts - 1].any() or not _refractory_after(sm, ts - 1, int(res.refractory_period)).any():
        return False
    burst = no_burst = False
    for i in res.out_idx:
        before, after = np.nonzero(sm[:ts, i])[0], np.nonzero(sm[ts:, i])[0]
        if len(before) and len(after):
            isi = ts + int(after[0]) - int(before[-1])
            burst |= isi <= int(res.burst_isi_max)
            no_burst |= isi > int(res.burst_isi_max)
    # (a refractory period above the burst limit makes every interval longer than the limit: no burst can straddle)
    return no_burst and (burst or int(res.refractory_period) >= int(res.burst_isi_max))


class _Case:
    """One reservoir, its rasters, the oracle's whole-clip results and the main cut; built once per module."""

    def __init__(self, oracle_c, shape_index, refractory):
        from lsm_speech_classifier_amd import reservoir as R, snn
        n, k, n_out, c = SHAPES[shape_index]
        self.res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                        mean_weight=2.0 / (k // 2), refractory_period=refractory), c)
        self.rasters = _rasters(shape_index, c)
        self.ref = {}
        for keys in (ALL_KEYS, TWO_KEYS):
            rows = []
            for r in self.rasters:
                f, sm, vt = oracle_c.lif_run(self.res, r, keys, want_trace=True)
                per = sm.sum(axis=0, dtype=np.int64)
                rows.append((f, sm, vt, [int(np.count_nonzero(per)), int(per.sum())]))
            self.ref[tuple(keys)] = rows
        sms = [row[1] for row in self.ref[tuple(ALL_KEYS)]]
        self.t_star = next((ts for ts in range(T // 2, T - 2)
                            if all(_cut_is_through_activity(sm, self.res, ts) for sm in sms)), None)
        assert self.t_star is not None, (
            f"shape {SHAPES[shape_index]}: no step in [{T // 2}, {T - 2}) at which every clip has spikes at the step before, "
            f"refractory neurons, and output neurons straddling the cut with and without a burst interval")
        self.net = snn.SNN(None, reservoir=self.res)
        self.offered = []
        from lsm_speech_classifier_amd import _lib
        for kernel in KERNELS:
            try:
                self.net.set_kernel(kernel)
                self.offered.append(kernel)
            except _lib.LsmHipError:
                pass
        self.net.set_kernel("auto")
        assert self.offered, "no kernel family offered"


_CASES = {}


def _case(oracle_c, shape_index, refractory=2):
    key = (shape_index, refractory)
    if key not in _CASES:
        _CASES[key] = _Case(oracle_c, shape_index, refractory)
    return _CASES[key]


def _continued(case, cuts, keys=ALL_KEYS, kernels=None, wpcs=None, in_place=True, longest_first=False, rasters=None):
    """The clips in len(cuts) - 1 launches over steps [cuts[i], cuts[i + 1]); launch i runs on kernels[i % len] with
    wpcs[i % len] waves per clip.  Returns (features, spike matrix, trace, statistics, state) as the last launch and
    the concatenation of the per-launch outputs give them."""
    import torch
    net = case.net
    r = torch.from_numpy(case.rasters if rasters is None else rasters).cuda()
    n = r.shape[0]
    stats = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    state = net.new_state(n)
    feats, sms, vts = None, [], []
    for i, (t0, t1) in enumerate(zip(cuts[:-1], cuts[1:])):
        if kernels:
            net.set_kernel(kernels[i % len(kernels)])
            _RAN.add(kernels[i % len(kernels)])
        assert state.steps_done == t0
        nxt = state if in_place else net.new_state(n)
        if not in_place:
            nxt.data.fill_(0xA5)                    # an out-of-place state is written in full, whatever it held
        feats, sm, vt = net.run_batch(r[:, :, t0:t1], keys, want_spike_matrix=True, want_v_trace=True,
                                      waves_per_clip=wpcs[i % len(wpcs)] if wpcs else 0, stats_out=stats,
                                      longest_first=longest_first, state=state, state_out=None if in_place else nxt)
        state = nxt
        sms.append(sm)
        vts.append(vt)
    net.set_kernel("auto")
    return feats.cpu().numpy(), torch.cat(sms, 1).cpu().numpy(), torch.cat(vts, 1).cpu().numpy(), stats.cpu().numpy(), state


def _assert_whole_clip(got, ref, msg):
    f, sm, vt, stats = got[:4]
    for b, (f_ref, sm_ref, vt_ref, st_ref) in enumerate(ref):
        np.testing.assert_array_equal(sm[b], sm_ref, err_msg=f"spike matrix, clip {b}, {msg}")
        np.testing.assert_array_equal(vt[b], vt_ref, err_msg=f"membrane trace, clip {b}, {msg}")
        np.testing.assert_array_equal(f[b], f_ref, err_msg=f"features, clip {b}, {msg}")
        assert stats[b].tolist() == st_ref, f"statistics, clip {b}, {msg}"


def _waves_offered(case, kernel):
    from lsm_speech_classifier_amd import _lib
    case.net.set_kernel(kernel)
    out = []
    for wpc in (1, 2, 4, 8, 16):
        try:
            case.net.plan(B, T, wpc)
            out.append(wpc)
        except _lib.LsmHipError as e:
            assert "layout" in str(e), str(e)
    case.net.set_kernel("auto")
    return out


SHAPE_IDS = [f"N{n}-C{c}" for n, _, _, c in SHAPES]


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_cut_runs_equal_the_whole_clip(torch_cuda, oracle_c, shape_index):
    """Two launches cut at t*, cuts after the first and before the last step, 14 launches of 7 steps and 96 launches of
    one step, on every family: features, spike matrix, trace and statistics of the oracle's whole clip."""
    case = _case(oracle_c, shape_index)
    ref = case.ref[tuple(ALL_KEYS)]
    sevens = list(range(0, T, 7)) + [T]
    assert len(sevens) - 1 == 14
    for kernel in case.offered:
        for cuts in ([0, case.t_star, T], [0, 1, T - 1, T], sevens):
            _assert_whole_clip(_continued(case, cuts, kernels=[kernel]), ref, f"kernel {kernel}, cuts {cuts}")
        _assert_whole_clip(_continued(case, [0, case.t_star, T], TWO_KEYS, kernels=[kernel]), case.ref[tuple(TWO_KEYS)],
                           f"kernel {kernel}, two keys")
    # one step per launch: the state is everything a launch knows (the library's own choice of kernel)
    _assert_whole_clip(_continued(case, list(range(T + 1))), ref, "one step per launch")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_zero_state_is_reset_and_in_place_equals_out_of_place(torch_cuda, oracle_c, shape_index):
    import torch
    case = _case(oracle_c, shape_index)
    ref = case.ref[tuple(ALL_KEYS)]
    for kernel in case.offered:
        case.net.set_kernel(kernel)
        stats = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
        f, sm, vt = case.net.run_batch(case.rasters, ALL_KEYS, want_spike_matrix=True, want_v_trace=True, stats_out=stats)
        plain = (f.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy(), stats.cpu().numpy())
        _assert_whole_clip(plain, ref, f"kernel {kernel}, no state")
        whole = _continued(case, [0, T], kernels=[kernel])
        for a, b_ in zip(plain, whole[:4]):
            np.testing.assert_array_equal(a, b_, err_msg=f"kernel {kernel}: new_state + first_step 0 against no state")
        inp = _continued(case, [0, case.t_star, T], kernels=[kernel])
        outp = _continued(case, [0, case.t_star, T], kernels=[kernel], in_place=False)
        _assert_whole_clip(outp, ref, f"kernel {kernel}, out of place")
        assert torch.equal(inp[4].data, outp[4].data), f"kernel {kernel}: state in place against out of place"
        assert inp[4].steps_done == outp[4].steps_done == T


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_hand_over_between_families(torch_cuda, oracle_c, shape_index):
    """The state does not depend on the kernel that wrote it: every ordered pair of families, cut at t*."""
    import torch
    case = _case(oracle_c, shape_index)
    ref = case.ref[tuple(ALL_KEYS)]
    states = {}
    for first in case.offered:
        for second in case.offered:
            got = _continued(case, [0, case.t_star, T], kernels=[first, second])
            _assert_whole_clip(got, ref, f"{first} then {second}")
            states[(first, second)] = got[4].data
    one = next(iter(states.values()))
    for pair, data in states.items():
        assert torch.equal(data, one), f"state after {pair[0]} then {pair[1]} differs from the other families'"


@pytest.mark.parametrize("shape_index,refractory", [(i, 2) for i in range(len(SHAPES))] + [(0, 7)],
                         ids=SHAPE_IDS + ["N256-C40-refractory7"])
def test_state_accessors(torch_cuda, oracle_c, shape_index, refractory):
    case = _case(oracle_c, shape_index, refractory)
    ref = case.ref[tuple(ALL_KEYS)]
    ts = case.t_star
    for kernel in case.offered:
        state = _continued(case, [0, ts], kernels=[kernel])[4]
        assert state.steps_done == ts
        v, rf, last = state.membrane().cpu().numpy(), state.refractory().cpu().numpy(), state.last_spikes().cpu().numpy()
        ever, total = state.ever_fired().cpu().numpy(), state.spike_total().cpu().numpy()
        deepest = 0
        for b, (_, sm, vt, _) in enumerate(ref):
            np.testing.assert_array_equal(v[b], vt[ts - 1], err_msg=f"membrane, clip {b}, {kernel}")
            np.testing.assert_array_equal(last[b], sm[ts - 1].astype(bool), err_msg=f"last spikes, clip {b}, {kernel}")
            want = _refractory_after(sm, ts - 1, refractory)
            assert want.any()
            deepest = max(deepest, int(want.max()))
            np.testing.assert_array_equal(rf[b], want, err_msg=f"refractory, clip {b}, {kernel}")
            np.testing.assert_array_equal(ever[b], sm[:ts].any(axis=0), err_msg=f"ever fired, clip {b}, {kernel}")
            assert int(total[b]) == int(sm[:ts].sum(dtype=np.int64))
        assert deepest == refractory or deepest > 2          # period 7: countdowns the mask form of period 2 cannot hold
        whole = _continued(case, [0, ts, T], kernels=[kernel])
        _assert_whole_clip(whole, ref, f"kernel {kernel}, refractory {refractory}")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_waves_per_clip_change_between_launches(torch_cuda, oracle_c, shape_index):
    case = _case(oracle_c, shape_index)
    ref = case.ref[tuple(ALL_KEYS)]
    for kernel in case.offered:
        waves = _waves_offered(case, kernel)
        assert waves, f"{kernel}: no forced layout"
        # every layout hands over to the next one (and the last to the first)
        for wa, wb in zip(waves, waves[1:] + waves[:1]):
            got = _continued(case, [0, case.t_star, T], kernels=[kernel], wpcs=[wa, wb])
            _assert_whole_clip(got, ref, f"kernel {kernel}, waves per clip {wa} then {wb}")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_ordered_start(torch_cuda, oracle_c, shape_index):
    """`order_workspace` given: three clips are fewer than the compute units and start as they are; at the smallest
    reservoir a batch of more clips than compute units really starts longest first (the state of clip b is block b)."""
    import torch
    case = _case(oracle_c, shape_index)
    ref = case.ref[tuple(ALL_KEYS)]
    for kernel in case.offered:
        _assert_whole_clip(_continued(case, [0, case.t_star, T], kernels=[kernel], longest_first=True), ref,
                           f"kernel {kernel}, ordered")
    if shape_index == 0:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        reps = cus // B + 1
        many = np.ascontiguousarray(np.tile(case.rasters, (reps, 1, 1)))
        assert len(many) > cus and len({int(r.sum()) for r in case.rasters}) == B      # more clips than CUs, keys differ
        for kernel in case.offered:
            got = _continued(case, [0, case.t_star, T], kernels=[kernel], longest_first=True, rasters=many)
            _assert_whole_clip(got, ref * reps, f"kernel {kernel}, {len(many)} clips ordered")


def test_refusals(torch_cuda, oracle_c):
    import ctypes as C
    import torch
    from lsm_speech_classifier_amd import _lib
    case = _case(oracle_c, 0)
    net = case.net
    r = torch.from_numpy(case.rasters).cuda()
    state = net.new_state(B)
    state.steps_done = 65536 - T
    with pytest.raises(_lib.LsmHipError, match="first_step"):
        net.run_batch(r, ALL_KEYS, state=state)
    state.steps_done = 65535 - T                                # the last run the ABI accepts is accepted
    net.run_batch(r, ['spike_counts'], state=state)
    assert state.steps_done == 65535
    # first_step = 5 without a state: only the C entry point can be asked that
    feats = torch.empty((B, 8 * len(case.res.out_idx)), dtype=torch.float32, device="cuda")
    keys = np.arange(8, dtype=np.int32)
    rc = net.lib.lsm_reservoir_run_from(net._handle, C.c_void_p(r.data_ptr()), B, T, 5, None, None,
                                        C.c_void_p(keys.ctypes.data), 8, C.c_void_p(feats.data_ptr()), None, None, None, 0,
                                        None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1
    with pytest.raises(_lib.LsmHipError, match="first_step"):
        _lib.check(rc, "lsm_reservoir_run_from")
    rc = net.lib.lsm_reservoir_run_from(net._handle, C.c_void_p(r.data_ptr()), B, T, -1, None, None,
                                        C.c_void_p(keys.ctypes.data), 8, C.c_void_p(feats.data_ptr()), None, None, None, 0,
                                        None, 0, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.LsmHipError, match="first_step"):
        _lib.check(rc, "lsm_reservoir_run_from")
    good = net.new_state(B)
    rc = net.lib.lsm_reservoir_run_from(net._handle, C.c_void_p(r.data_ptr()), B, T, 0, C.c_void_p(good.data.data_ptr() + 4),
                                        None, C.c_void_p(keys.ctypes.data), 8, C.c_void_p(feats.data_ptr()), None, None, None,
                                        0, None, 0, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.LsmHipError, match="state_in"):
        _lib.check(rc, "lsm_reservoir_run_from")
    for bad in (net.new_state(B + 1), net.new_state(B).clone()):
        if bad.data.shape[0] == B:
            bad.data = bad.data.cpu()                          # right size, wrong device
        with pytest.raises(_lib.LsmHipError, match="state"):
            net.run_batch(r, ALL_KEYS, state=bad)
    short = net.new_state(B)
    short.data = short.data[:, :-16].contiguous()
    with pytest.raises(_lib.LsmHipError, match="state"):
        net.run_batch(r, ALL_KEYS, state=short)
    torch.cuda.synchronize()
    # the handle still works
    _assert_whole_clip(_continued(case, [0, case.t_star, T]), case.ref[tuple(ALL_KEYS)], "after the refusals")


def test_every_family_ran(torch_cuda):
    """Last in the module: over the four shapes every kernel family took part in a continued run."""
    missing = [kernel for kernel in KERNELS if kernel not in _RAN]
    assert not missing, f"kernel families that never ran a continued launch: {missing} (ran: {sorted(_RAN)})"
