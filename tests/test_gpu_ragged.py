"""Clips of different lengths in one reservoir launch (SPEC.md 4c, `lsm_reservoir_run_ragged`, `SNN.run_batch(lengths=...)`).

Clip b of a ragged launch must be, bit for bit, the launch over its own `L_b` steps alone.  The reference is the plain-C
oracle (oracle/lsm_oracle.c) on the raster TRUNCATED to `L_b` steps, one run per clip; the code under test is never its own
reference and nothing here has a tolerance.  Raster bytes behind a clip's length are poisoned (255) and every output is
pre-filled with sentinels (NaN features and trace, -1 statistics, 0xAB spike-matrix bytes), so a kernel that ignores the
lengths, reads past them or writes past them fails.  Every kernel family a reservoir offers runs (dense, sparse, pair
blocks, quads of both ownerships); the last test of the module fails when one of them never ran a ragged launch.

Before anything is compared the oracle's own output must show that the clips end inside activity: every clip of 37 steps
or more has an output-neuron spike at its last step and a reservoir spike within its last two steps (its neurons are
inside their refractory period when the clip ends)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
TWO_KEYS = ['burst_counts', 'spike_variances']              # a subset, not in the default order
KERNELS = ("dense", "sparse", "ring-pairs", "ring-quads", "ring-contiguous")
SHAPES = [(256, 50, 100, 40), (1024, 204, 410, 64), (1024, 204, 410, 160), (2048, 408, 820, 128)]   # (N, k, n_out, C)
SHAPE_IDS = [f"N{n}-C{c}" for n, _, _, c in SHAPES]
T, B, DENSITY, REFRACTORY = 96, 8, 0.35, 2
LENGTHS = [96, 0, 1, 37, 64, 95, 2, 50]
LENGTHS_95 = [95, 0, 1, 37, 64, 94, 2, 50]                  # stride 95: the byte path of the packing
_RAN = set()                                                # kernel families that ran at least one ragged launch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


# ----------------------------------------------------------------------------- helpers ----
def _last_fire(sm):
    """(N,) step of every neuron's last spike in the (L, N) spike matrix, -1 for a silent one."""
    steps = np.arange(1, sm.shape[0] + 1, dtype=np.int64)[:, None]
    return (sm.astype(np.int64) * steps).max(axis=0) - 1


def _refractory_after(sm, t, period):
    """Countdown of every neuron after step t, from the spike matrix: max(0, R - (t - t_last)) (tests/test_gpu_state.py)."""
    last = _last_fire(sm[:t + 1])
    return np.where(last >= 0, np.maximum(0, period - (t - last)), 0)


class _Case:
    """One reservoir, its 8 clips and the oracle's results on their truncations; built once per module."""

    def __init__(self, oracle_c, shape_index):
        from lsm_speech_classifier_amd import _lib, reservoir as R, snn
        n, k, n_out, c = SHAPES[shape_index]
        self.oracle = oracle_c
        self.res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                        mean_weight=2.0 / (k // 2), refractory_period=REFRACTORY), c)
        self.rasters = np.stack([(np.random.RandomState(7000 + 100 * shape_index + b).random_sample((c, T)) < DENSITY)
                                 .astype(np.uint8) for b in range(B)])
        self._ref = {}
        # the clips end inside activity (module docstring), from the oracle alone
        for b, length in enumerate(LENGTHS):
            if length >= 37:
                sm = self.ref(b, length, ALL_KEYS)[1]
                assert sm[length - 1, self.res.out_idx].any(), f"shape {shape_index} clip {b}: no output spike at its last step"
                assert sm[length - 2:length].any(), f"shape {shape_index} clip {b}: no reservoir spike in its last two steps"
                assert _refractory_after(sm, length - 1, REFRACTORY).any()
        self.net = snn.SNN(None, reservoir=self.res)
        self.offered = []
        for kernel in KERNELS:
            try:
                self.net.set_kernel(kernel)
                self.offered.append(kernel)
            except _lib.LsmHipError:
                pass
        self.net.set_kernel("auto")
        assert self.offered, "no kernel family offered"

    def ref(self, b, length, keys):
        """(features, spike matrix, trace, statistics) of the oracle on clip b's first `length` steps (shared, read-only)."""
        key = (b, length, tuple(keys))
        if key not in self._ref:
            f, sm, vt = self.oracle.lif_run(self.res, np.ascontiguousarray(self.rasters[b][:, :length]), keys, want_trace=True)
            per = sm.sum(axis=0, dtype=np.int64)
            for a in (f, sm, vt):
                a.setflags(write=False)
            self._ref[key] = (f, sm, vt, [int(np.count_nonzero(per)), int(per.sum())])
        return self._ref[key]

    def waves(self, kernel, n_clips=B, n_steps=T):
        """(the default plan's waves per clip, one other forced layout of this family or None)."""
        from lsm_speech_classifier_amd import _lib
        self.net.set_kernel(kernel)
        default = self.net.plan(n_clips, n_steps, 0)["waves_per_clip"]
        other = None
        for wpc in (16, 8, 4, 2, 1):
            if wpc != default and other is None:
                try:
                    self.net.plan(n_clips, n_steps, wpc)
                    other = wpc
                except _lib.LsmHipError as e:
                    assert "layout" in str(e), str(e)
        self.net.set_kernel("auto")
        return default, other


_CASES = {}


def _case(oracle_c, shape_index):
    if shape_index not in _CASES:
        _CASES[shape_index] = _Case(oracle_c, shape_index)
    return _CASES[shape_index]


def _poisoned(rasters, lengths):
    """The rasters with every byte at t >= L_b set to 255."""
    out = rasters.copy()
    for b, length in enumerate(lengths):
        out[b, :, length:] = 255
    return out


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _launch(net, rasters, steps, keys, wpc=0, first_step=0, state_in=None, state_out=None, ordered=False):
    """One lsm_reservoir_run_ragged call into sentinel-filled outputs.  rasters: uint8 (n, C, stride) NumPy; steps: int
    list / array, an int32 device tensor, or None (NULL).  Returns NumPy (features, spike matrix, trace, statistics) and
    the order workspace (or None)."""
    import torch
    from lsm_speech_classifier_amd import _lib, snn
    r = torch.from_numpy(np.ascontiguousarray(rasters)).cuda()
    n, _, stride = r.shape
    if steps is not None and not isinstance(steps, torch.Tensor):
        steps = torch.tensor([int(x) for x in steps], dtype=torch.int32, device="cuda")
    n_out, n_neu = net.num_output_neurons, net.num_neurons
    feats = torch.full((n, len(keys) * n_out), float("nan"), dtype=torch.float32, device="cuda")
    sm = torch.full((n, stride, n_neu), 0xAB, dtype=torch.uint8, device="cuda")
    vt = torch.full((n, stride, n_neu), float("nan"), dtype=torch.float32, device="cuda")
    stats = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    key_ids = np.array([snn.FEATURE_KEYS.index(k) for k in keys], dtype=np.int32)
    need = net.lib.lsm_reservoir_order_workspace(n) if ordered else 0
    ws = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda") if ordered else None
    rc = net.lib.lsm_reservoir_run_ragged(
        net._handle, _ptr(r), n, stride, _ptr(steps), first_step, _ptr(state_in), _ptr(state_out),
        C.c_void_p(key_ids.ctypes.data), len(keys), _ptr(feats), _ptr(sm), _ptr(vt), _ptr(stats), wpc, _ptr(ws), need,
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "lsm_reservoir_run_ragged")
    torch.cuda.synchronize()
    return (feats.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy(), stats.cpu().numpy(),
            ws.cpu().numpy() if ordered else None)


def _assert_clip(got, b, length, ref, msg, sentinels=True):
    """Row b of a launch's outputs against the oracle's run over `length` steps; rows from `length` on and a clip of no
    steps keep their sentinels."""
    f, sm, vt, stats = got[:4]
    if length == 0:
        assert np.isnan(f[b]).all(), f"features of the zero-step clip {b} were written, {msg}"
        assert stats[b].tolist() == [-1, -1], f"statistics of the zero-step clip {b} were written, {msg}"
    else:
        f_ref, sm_ref, vt_ref, st_ref = ref
        np.testing.assert_array_equal(sm[b, :length], sm_ref, err_msg=f"spike matrix, clip {b}, {msg}")
        np.testing.assert_array_equal(vt[b, :length], vt_ref, err_msg=f"membrane trace, clip {b}, {msg}")
        np.testing.assert_array_equal(f[b], f_ref, err_msg=f"features, clip {b}, {msg}")
        assert stats[b].tolist() == st_ref, f"statistics, clip {b}, {msg}"
    if sentinels:
        assert (sm[b, length:] == 0xAB).all(), f"spike-matrix rows from {length} on were written, clip {b}, {msg}"
        assert np.isnan(vt[b, length:]).all(), f"trace rows from {length} on were written, clip {b}, {msg}"


def _assert_launch(case, got, lengths, keys, msg):
    for b, length in enumerate(lengths):
        _assert_clip(got, b, length, case.ref(b, length, keys) if length else None, msg)


def _assert_continued(got, b, ref, t0, n, msg):
    """Row b of a launch over the steps [t0, t0 + n) of a run the oracle made from step 0: cumulative features and
    statistics, this launch's rows of the spike matrix and the trace."""
    f, sm, vt, stats = got[:4]
    f_ref, sm_ref, vt_ref, st_ref = ref
    np.testing.assert_array_equal(sm[b, :n], sm_ref[t0:t0 + n], err_msg=f"spike matrix, clip {b}, {msg}")
    np.testing.assert_array_equal(vt[b, :n], vt_ref[t0:t0 + n], err_msg=f"membrane trace, clip {b}, {msg}")
    np.testing.assert_array_equal(f[b], f_ref, err_msg=f"features, clip {b}, {msg}")
    assert stats[b].tolist() == st_ref, f"statistics, clip {b}, {msg}"


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_every_clip_is_its_own_launch(torch_cuda, oracle_c, shape_index):
    """Every family, the default layout and one other, all keys and two: rows below L_b are the oracle's on the truncated
    raster, everything else keeps its sentinel."""
    case = _case(oracle_c, shape_index)
    poisoned = _poisoned(case.rasters, LENGTHS)
    for kernel in case.offered:
        for wpc in (0, case.waves(kernel)[1]):                  # the library's own layout, and one other
            if wpc is None:
                continue
            case.net.set_kernel(kernel)
            for keys in (ALL_KEYS, TWO_KEYS):
                got = _launch(case.net, poisoned, LENGTHS, keys, wpc)
                _assert_launch(case, got, LENGTHS, keys, f"kernel {kernel}, waves per clip {wpc}, {len(keys)} keys")
            _RAN.add(kernel)
    case.net.set_kernel("auto")


def test_stride_that_is_no_multiple_of_four(torch_cuda, oracle_c):
    """Stride 95: the raster is packed byte by byte.  One shape per family (the first that offers it)."""
    seen = set()
    for shape_index in range(len(SHAPES)):
        case = _case(oracle_c, shape_index)
        todo = [k for k in case.offered if k not in seen]
        if not todo:
            continue
        short = np.ascontiguousarray(case.rasters[:, :, :95])            # (the oracle's truncations are prefixes of these too)
        poisoned = _poisoned(short, LENGTHS_95)
        for kernel in todo:
            case.net.set_kernel(kernel)
            got = _launch(case.net, poisoned, LENGTHS_95, ALL_KEYS)
            _assert_launch(case, got, LENGTHS_95, ALL_KEYS, f"stride 95, kernel {kernel}, shape {SHAPES[shape_index]}")
            seen.add(kernel)
        case.net.set_kernel("auto")
    assert seen == set(KERNELS), f"families without a shape: {set(KERNELS) - seen}"


def _assert_final_states(case, state, lengths, msg):
    """Each clip's state is what the oracle's trace and spike matrix imply after its step L_b - 1 (zeros: no step)."""
    v, rf, last = state.membrane().cpu().numpy(), state.refractory().cpu().numpy(), state.last_spikes().cpu().numpy()
    ever, total = state.ever_fired().cpu().numpy(), state.spike_total().cpu().numpy()
    for b, length in enumerate(lengths):
        if length == 0:
            assert not state.data[b].any().item(), f"state of the zero-step clip {b} is not reset(), {msg}"
            continue
        _, sm, vt, _ = case.ref(b, length, ALL_KEYS)
        np.testing.assert_array_equal(v[b], vt[length - 1], err_msg=f"membrane, clip {b}, {msg}")
        np.testing.assert_array_equal(last[b], sm[length - 1].astype(bool), err_msg=f"last spikes, clip {b}, {msg}")
        np.testing.assert_array_equal(rf[b], _refractory_after(sm, length - 1, REFRACTORY), err_msg=f"refractory, clip {b}, {msg}")
        np.testing.assert_array_equal(ever[b], sm.any(axis=0), err_msg=f"ever fired, clip {b}, {msg}")
        assert int(total[b]) == int(sm.sum(dtype=np.int64)), f"spike total, clip {b}, {msg}"


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_run_chunked_with_lengths(torch_cuda, oracle_c, shape_index):
    """Launches of 40, 40 and 16 steps; clips end inside the first, the second and the third and ride along with 0 steps
    afterwards.  `run_chunked` itself, then the same launches on alternating kernel families."""
    import torch
    from lsm_speech_classifier_amd import snn
    case = _case(oracle_c, shape_index)
    net = case.net
    chunks = snn.ragged_chunks(LENGTHS, 40)
    assert [(t0, n) for t0, n, _ in chunks] == [(0, 40), (40, 40), (80, 16)]
    ends = [next(k for k, (_, n, s) in enumerate(chunks) if s[b] < n) if L < T else 2 for b, L in enumerate(LENGTHS)]
    assert {0, 1, 2} <= set(ends)
    poisoned = torch.from_numpy(_poisoned(case.rasters, LENGTHS)).cuda()
    stats = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    f, sm, vt, state = net.run_chunked(poisoned, ALL_KEYS, chunk_steps=40, want_spike_matrix=True, want_v_trace=True,
                                       stats_out=stats, lengths=LENGTHS, want_state=True)
    got = (f.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy(), stats.cpu().numpy())
    assert state.steps_done == T and state.ended.tolist() == [L < T for L in LENGTHS]
    for b, length in enumerate(LENGTHS):
        if length:
            _assert_clip(got, b, length, case.ref(b, length, ALL_KEYS), "run_chunked", sentinels=False)
        else:           # outputs the wrapper allocates start as zeros; the caller's statistics row is not touched
            assert not got[0][b].any() and got[3][b].tolist() == [-1, -1]
        assert not got[1][b, length:].any() and not got[2][b, length:].any(), f"rows past the length of clip {b} are not zero"
    _assert_final_states(case, state, LENGTHS, "run_chunked")

    # the same launches by hand, every launch on the next family
    fams = case.offered
    feats = torch.full((B, 8 * net.num_output_neurons), float("nan"), dtype=torch.float32, device="cuda")
    stats.fill_(-1)
    st = net.new_state(B)
    for i, (t0, n, steps) in enumerate(chunks):
        net.set_kernel(fams[i % len(fams)])
        _RAN.add(fams[i % len(fams)])
        assert st.steps_done == t0
        net.run_batch(poisoned[:, :, t0:t0 + n], ALL_KEYS, stats_out=stats, features_out=feats, state=st, lengths=steps)
    net.set_kernel("auto")
    f2, s2 = feats.cpu().numpy(), stats.cpu().numpy()
    for b, length in enumerate(LENGTHS):
        if length:
            f_ref, _, _, st_ref = case.ref(b, length, ALL_KEYS)
            np.testing.assert_array_equal(f2[b], f_ref, err_msg=f"features, clip {b}, alternating {fams}")
            assert s2[b].tolist() == st_ref
        else:
            assert np.isnan(f2[b]).all() and s2[b].tolist() == [-1, -1]
    _assert_final_states(case, st, LENGTHS, f"alternating {fams}")
    assert torch.equal(st.data, state.data), "the state depends on the families that ran"


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_zero_step_clips_hand_their_state_on(torch_cuda, oracle_c, shape_index):
    """A clip of no steps: state_out receives its state_in block byte for byte (the real state after 40 steps), nothing
    happens in place, and without state_in the block is zeros -- on every family."""
    import torch
    case = _case(oracle_c, shape_index)
    net = case.net
    r = case.rasters
    zero = [1, 4]
    steps = [0 if b in zero else 40 for b in range(B)]
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        first = net.new_state(B)
        net.run_batch(r[:, :, :40], ['spike_counts'], state=first)              # every clip: the real state after 40 steps
        assert all(first.data[b].any().item() for b in range(B))
        # distinct blocks
        out = net.new_state(B)
        out.data.fill_(0xA5)
        got = _launch(net, r[:, :, 40:80], steps, ALL_KEYS, first_step=40, state_in=first.data, state_out=out.data)
        for b in range(B):
            if b in zero:
                assert torch.equal(out.data[b], first.data[b]), f"{kernel}: zero-step clip {b}, state not copied"
                _assert_clip(got, b, 0, None, f"{kernel}, zero-step clip with a state")
            else:
                _assert_continued(got, b, case.ref(b, 80, ALL_KEYS), 40, 40, f"{kernel}, continued beside zero-step clips")
        # in place
        same = first.clone()
        _launch(net, r[:, :, 40:80], steps, ALL_KEYS, first_step=40, state_in=same.data, state_out=same.data)
        for b in range(B):
            if b in zero:
                assert torch.equal(same.data[b], first.data[b]), f"{kernel}: zero-step clip {b} changed in place"
            else:
                assert torch.equal(same.data[b], out.data[b]), f"{kernel}: clip {b} in place against out of place"
        # no state_in: reset
        fresh = net.new_state(B)
        fresh.data.fill_(0xA5)
        _launch(net, r[:, :, :40], steps, ALL_KEYS, state_in=None, state_out=fresh.data)
        for b in range(B):
            if b in zero:
                assert not fresh.data[b].any().item(), f"{kernel}: zero-step clip {b} without state_in is not zeros"
            else:
                assert torch.equal(fresh.data[b], first.data[b]), f"{kernel}: clip {b} from reset"
    net.set_kernel("auto")


def test_clamping_and_refusals(torch_cuda, oracle_c):
    import torch
    case = _case(oracle_c, 0)
    net = case.net
    # device values outside [0, n_steps] behave as 0 and n_steps
    wild = [-5, 1000, 96, 0, 37, -2147483648, 2147483647, 50]
    clamped = [min(max(x, 0), T) for x in wild]
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        got = _launch(net, _poisoned(case.rasters, clamped), wild, ALL_KEYS)
        _assert_launch(case, got, clamped, ALL_KEYS, f"kernel {kernel}, lengths {wild}")
        # clip_steps = NULL: every clip runs the whole stride
        got = _launch(net, case.rasters, None, ALL_KEYS)
        _assert_launch(case, got, [T] * B, ALL_KEYS, f"kernel {kernel}, no lengths")
    net.set_kernel("auto")
    # the same through run_batch with a device tensor (never read back), rows past the lengths are zeros
    dev = torch.tensor(wild, dtype=torch.int32, device="cuda")
    f, sm, vt = net.run_batch(_poisoned(case.rasters, clamped), ALL_KEYS, want_spike_matrix=True, want_v_trace=True, lengths=dev)
    f, sm, vt = f.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy()
    for b, length in enumerate(clamped):
        assert not sm[b, length:].any() and not vt[b, length:].any()
        if length:
            np.testing.assert_array_equal(f[b], case.ref(b, length, ALL_KEYS)[0])
            np.testing.assert_array_equal(sm[b, :length], case.ref(b, length, ALL_KEYS)[1])
        else:
            assert not f[b].any()
    # host values are checked before anything is launched
    for bad in ([97] + [0] * 7, [-1] + [0] * 7, np.array([96] * 7 + [1000]), [1, 2, 3], [1.5] * 8):
        with pytest.raises(ValueError, match="lengths"):
            net.run_batch(case.rasters, ALL_KEYS, lengths=bad)
    # a clip that ran short has ended
    st = net.new_state(B)
    net.run_batch(case.rasters[:, :, :40], ALL_KEYS, state=st, lengths=[40, 0, 1, 37, 40, 40, 2, 40])
    assert st.ended.tolist() == [False, True, True, True, False, False, True, False] and st.steps_done == 40
    before = st.data.clone()
    with pytest.raises(ValueError, match="ended"):
        net.run_batch(case.rasters[:, :, 40:80], ALL_KEYS, state=st, lengths=[40, 0, 0, 1, 24, 40, 0, 10])
    assert st.steps_done == 40 and torch.equal(st.data, before)             # refused before the launch
    net.run_batch(case.rasters[:, :, 40:80], ALL_KEYS, state=st, lengths=[40, 0, 0, 0, 24, 40, 0, 10])
    assert st.steps_done == 80 and st.ended.tolist() == [False, True, True, True, True, False, True, True]


def test_ordered_ragged_launch(torch_cuda, oracle_c):
    """More clips than compute units and the order workspace: clips are ranked by their input spikes inside their own
    lengths (the poison behind them does not count), zero-step clips start last, and row b is still clip b's."""
    torch = torch_cuda
    case = _case(oracle_c, 0)
    net = case.net
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus + 37
    lengths = [LENGTHS[i % B] for i in range(n)]
    many = np.ascontiguousarray(case.rasters[[i % B for i in range(n)]])
    poisoned = _poisoned(many, lengths)
    keys_want = np.array([int(np.count_nonzero(many[i][:, :lengths[i]])) for i in range(n)], dtype=np.int32)
    order_want = np.argsort(-keys_want.astype(np.int64), kind="stable").astype(np.int32)
    silent = [i for i in range(n) if keys_want[i] == 0]
    assert n <= 4096 and silent == [i for i in range(n) if lengths[i] == 0] and order_want[-len(silent):].tolist() == silent
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        got = _launch(net, poisoned, lengths, ALL_KEYS, ordered=True)
        np.testing.assert_array_equal(got[4][:n], keys_want, err_msg=f"{kernel}: keys of the ragged clips")
        np.testing.assert_array_equal(got[4][n:], order_want, err_msg=f"{kernel}: start order")
        for i, length in enumerate(lengths):
            _assert_clip(got, i, length, case.ref(i % B, length, ALL_KEYS) if length else None, f"{kernel}, ordered, clip {i}")
    net.set_kernel("auto")


def test_features_from_recordings(torch_cuda, oracle_c):
    """Five recordings of 1, 3, 2, 1 and 4 windows in one batch: each row is the oracle's run over that recording's
    concatenated rasters (the front end is existing code and is not under test here)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
    windows = [1, 3, 2, 1, 4]
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    res = R.build_reservoir(R.SimulationParams(num_neurons=256, num_output_neurons=100, small_world_graph_k=50,
                                               mean_weight=2.0 / 25, refractory_period=2), fe.n_channels)
    net = snn.SNN(None, reservoir=res)
    clips = synth.class_chirps([0, 5, 9, 3, 7, 11, 2, 4, 6, 8, 10], seed=31)     # (11, n_samples)
    assert clips.shape == (sum(windows), fe.n_samples)
    rasters = fe.encode(torch.from_numpy(clips).cuda()).cpu().numpy()             # (11, C, n_steps), window by window
    recordings, first = [], 0
    for w in windows:
        recordings.append(np.ascontiguousarray(clips[first:first + w].reshape(-1)))
        first += w
    got = pipeline.features_from_recordings(recordings, fe, net, ALL_KEYS)
    assert tuple(got.shape) == (len(windows), 8 * 100) and got.is_cuda
    got = got.cpu().numpy()
    first = 0
    for r, w in enumerate(windows):
        whole = np.ascontiguousarray(np.concatenate(list(rasters[first:first + w]), axis=1))
        assert whole.shape == (fe.n_channels, w * fe.n_steps)
        f_ref, sm_ref, _ = oracle_c.lif_run(res, whole, ALL_KEYS)
        assert sm_ref[:, res.out_idx].any()
        np.testing.assert_array_equal(got[r], f_ref, err_msg=f"recording {r} of {w} windows")
        first += w
    two = pipeline.features_from_recordings(recordings[1:3], fe, net, TWO_KEYS).cpu().numpy()
    np.testing.assert_array_equal(two[0], got[1].reshape(8, 100)[[7, 1]].reshape(-1))
    np.testing.assert_array_equal(two[1], got[2].reshape(8, 100)[[7, 1]].reshape(-1))
    for bad, index in (([recordings[0], recordings[1][:-1]], 1), ([recordings[0][:10]], 0), ([np.zeros((2, fe.n_samples), np.float32)], 0)):
        with pytest.raises(ValueError, match=f"recording {index}"):
            pipeline.features_from_recordings(bad, fe, net, ALL_KEYS)


def test_every_family_ran(torch_cuda):
    """Last in the module: over the four shapes every kernel family ran a ragged launch."""
    missing = [kernel for kernel in KERNELS if kernel not in _RAN]
    assert not missing, f"kernel families that never ran a ragged launch: {missing} (ran: {sorted(_RAN)})"
