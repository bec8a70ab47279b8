"""Features per time segment and sliding window from one reservoir launch (SPEC.md 4b, `lsm_reservoir_run_segments`,
`lsm_segment_features`, `SNN.run_segments`, `pipeline.HotPath(time_segments=K)`,
`pipeline.sliding_features_from_long_audio`).

Every comparison is exact.  The reference is the plain-C oracle (oracle/lsm_oracle.c) on the WHOLE raster, computed once
per reservoir by tests/test_gpu_state.py's cases (the same reservoirs, rasters and kernel list), sliced on the host and
turned into rows by the oracle's own `spike_features`; the code under test is never its own reference.  Every kernel
family a reservoir offers runs; the last test of the module fails when one of them never ran a segmented launch.

Before anything is compared the oracle's own output must show that the cuts go through activity (`_assert_precondition`):
at every segment length with a boundary (24, 32, 8, 1) some output neuron's interval straddles a boundary with a burst
interval and some with a longer one, and some (segment, output neuron) pair has exactly one spike; a silent pair exists
at 24, 8 and 1.  (At S = 32 every output neuron of the three larger reservoirs fires in every third of every clip -- 0
silent pairs in the oracle's matrices -- so the silent pair is asserted where the rasters the issue fixes have one.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
TWO_KEYS = ['burst_counts', 'spike_variances']              # a subset, not in the default order
SEGMENT_STEPS = (24, 32, 8, 1, 96)
_RAN = set()                                                # kernel families that ran at least one segmented launch
_DENSE_FORMS = set()                                        # "registers" / "lds": record forms the dense kernel ran with


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _base():
    import test_gpu_state as base                           # SHAPES, T, B, KERNELS, the cached cases
    return base


# ------------------------------------------------------------------------ the reference ----
def _assert_precondition(case, base):
    sms = [row[1] for row in case.ref[tuple(ALL_KEYS)]]
    limit = int(case.res.burst_isi_max)
    for S in (24, 32, 8, 1):
        burst = longer = silent = single = 0
        for sm in sms:
            so = sm[:, case.res.out_idx]
            per_segment = so.reshape(base.T // S, S, -1).sum(axis=1)
            silent += int((per_segment == 0).sum())
            single += int((per_segment == 1).sum())
            for o in range(so.shape[1]):
                times = np.nonzero(so[:, o])[0]
                cross = (times[:-1] // S) != (times[1:] // S)
                isi = np.diff(times)[cross]
                burst += int((isi <= limit).sum())
                longer += int((isi > limit).sum())
        assert burst and longer, f"S={S}: {burst} burst and {longer} longer intervals straddle a segment boundary"
        assert single, f"S={S}: no (segment, output neuron) pair with exactly one spike"
        assert silent or S == 32, f"S={S}: no silent (segment, output neuron) pair"


def _case(oracle_c, shape_index):
    base = _base()
    case = base._case(oracle_c, shape_index)
    if not hasattr(case, "segment_rows"):
        _assert_precondition(case, base)
        case.segment_rows = {}
    return case


def _ref_rows(case, S, K=1, H=1, keys=ALL_KEYS, t_from=0, t_to=None):
    """(B, W, n_keys * n_out): the oracle's rows of the windows of K segments of S steps, hop H, over [t_from, t_to)."""
    from oracle import ref_numpy
    base = _base()
    t_to = base.T if t_to is None else t_to
    G = (t_to - t_from) // S
    out = []
    for b in range(base.B):
        sm = case.ref[tuple(ALL_KEYS)][b][1]
        rows = []
        for w in range((G - K) // H + 1):
            a, e = t_from + w * H * S, t_from + (w * H + K) * S
            d = case.segment_rows.get((b, a, e))
            if d is None:           # the oracle's spike_features on the slice, once per slice (all eight keys)
                d = case.segment_rows[(b, a, e)] = ref_numpy.spike_features(sm[a:e], case.res.out_idx,
                                                                            int(case.res.burst_isi_max))
            rows.append(np.concatenate([np.nan_to_num(d[k].copy()) for k in keys]))
        out.append(np.stack(rows))
    return np.stack(out)


def _run(case, kernel, S, keys=ALL_KEYS, K=1, H=1, wpc=0, **kw):
    case.net.set_kernel(kernel)
    _RAN.add(kernel)
    try:
        return case.net.run_segments(case.rasters, S, keys, K, H, waves_per_clip=wpc, **kw)
    finally:
        case.net.set_kernel("auto")


def _shape_ids():
    return [f"N{n}-C{c}" for n, _, _, c in [(256, 50, 100, 40), (1024, 204, 410, 64), (1024, 204, 410, 160),
                                            (2048, 408, 820, 128)]]


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("S", SEGMENT_STEPS)
@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_segment_rows_equal_the_oracle_on_slices(torch_cuda, oracle_c, shape_index, S):
    """K = 1: every (clip, segment) row, all eight keys and the two-key subset, on every family."""
    base = _base()
    assert _shape_ids() == base.SHAPE_IDS and base.T == 96 and base.B == 3
    case = _case(oracle_c, shape_index)
    n_out = len(case.res.out_idx)
    for keys in (ALL_KEYS, TWO_KEYS):
        want = _ref_rows(case, S, keys=keys)
        assert want.shape == (base.B, base.T // S, len(keys) * n_out)
        for kernel in case.offered:
            got = _run(case, kernel, S, keys)
            assert tuple(got.shape) == want.shape and got.dtype == torch_cuda.float32 and got.is_cuda
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"kernel {kernel}, S={S}, {len(keys)} keys")


@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_the_window_over_all_segments_is_the_whole_clip(torch_cuda, oracle_c, shape_index):
    """K = G from reset(): run_batch's row of the same clips and the C oracle's whole-clip row."""
    base = _base()
    case = _case(oracle_c, shape_index)
    for keys in (ALL_KEYS, TWO_KEYS):
        whole = np.stack([row[0] for row in case.ref[tuple(keys)]])
        for kernel in case.offered:
            case.net.set_kernel(kernel)
            plain = case.net.run_batch(case.rasters, keys)[0].cpu().numpy()
            np.testing.assert_array_equal(plain, whole, err_msg=f"kernel {kernel}: run_batch against the oracle")
            for S in SEGMENT_STEPS:
                got = _run(case, kernel, S, keys, K=base.T // S).cpu().numpy()
                assert got.shape == (base.B, 1, whole.shape[1])
                np.testing.assert_array_equal(got[:, 0], plain, err_msg=f"kernel {kernel}, S={S}, K=G against run_batch")


@pytest.mark.parametrize("K,H", [(2, 1), (3, 2)])
@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_sliding_windows_equal_the_oracle_on_their_slices(torch_cuda, oracle_c, shape_index, K, H):
    base = _base()
    case = _case(oracle_c, shape_index)
    S = 8
    want = _ref_rows(case, S, K, H)
    assert want.shape[1] == (base.T // S - K) // H + 1 == {(2, 1): 11, (3, 2): 5}[(K, H)]
    two = _ref_rows(case, S, K, H, TWO_KEYS)
    for kernel in case.offered:
        np.testing.assert_array_equal(_run(case, kernel, S, ALL_KEYS, K, H).cpu().numpy(), want,
                                      err_msg=f"kernel {kernel}, windows of {K} segments, hop {H}")
        np.testing.assert_array_equal(_run(case, kernel, S, TWO_KEYS, K, H).cpu().numpy(), two,
                                      err_msg=f"kernel {kernel}, windows of {K} segments, hop {H}, two keys")


def _one_launch(case, kernel, wpc, t0, t1, S, state, segmented, out_of_place=False):
    """Steps [t0, t1) from `state` (advanced in place unless out_of_place), segmented or through run_batch(state=...):
    (state bytes, cumulative features, statistics, spike matrix, trace, records or None, the new state)."""
    import torch
    net = case.net
    net.set_kernel(kernel)
    r = torch.from_numpy(case.rasters[:, :, t0:t1]).cuda()
    stats = torch.full((len(case.rasters), 2), -1, dtype=torch.int32, device="cuda")
    nxt = None
    if out_of_place:
        nxt = net.new_state(len(case.rasters))
        nxt.data.fill_(0xA5)
    rec = None
    if segmented:
        _RAN.add(kernel)
        rec, f, sm, vt = net.run_segment_records(r, S, ALL_KEYS, True, True, wpc, stats, False, state, nxt)
    else:
        f, sm, vt = net.run_batch(r, ALL_KEYS, want_spike_matrix=True, want_v_trace=True, waves_per_clip=wpc,
                                  stats_out=stats, longest_first=False, state=state, state_out=nxt)
    net.set_kernel("auto")
    new = nxt if out_of_place else state
    return new.data.clone(), f, stats, sm, vt, rec, new


@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_the_continuation_is_undisturbed(torch_cuda, oracle_c, shape_index):
    """A segmented launch with state / state_out gives the state bytes, cumulative features, statistics, spike matrix
    and trace of the same launch through run_batch(state=...), byte for byte -- both launches of a run cut at step 48,
    in place and out of place; two segmented launches on two different families and waves per clip give, concatenated,
    the records of one launch, and their rows are the oracle's."""
    torch = torch_cuda
    base = _base()
    case = _case(oracle_c, shape_index)
    S, cut = 24, 48
    names = ("state", "cumulative features", "statistics", "spike matrix", "membrane trace")
    for kernel in case.offered:
        for out_of_place in (False, True):
            st_seg, st_ref = case.net.new_state(base.B), case.net.new_state(base.B)
            for t0, t1 in ((0, cut), (cut, base.T)):
                seg = _one_launch(case, kernel, 0, t0, t1, S, st_seg, True, out_of_place)
                ref = _one_launch(case, kernel, 0, t0, t1, S, st_ref, False, out_of_place)
                for name, a, b_ in zip(names, seg[:5], ref[:5]):
                    assert torch.equal(a, b_), f"kernel {kernel}, steps [{t0}, {t1}), out of place {out_of_place}: {name}"
                st_seg, st_ref = seg[6], ref[6]
                assert st_seg.steps_done == st_ref.steps_done == t1
            # after the second launch: the oracle's whole clip
            second_half = [(f, sm[cut:], vt[cut:], st) for f, sm, vt, st in case.ref[tuple(ALL_KEYS)]]
            base._assert_whole_clip((seg[1].cpu().numpy(), seg[3].cpu().numpy(), seg[4].cpu().numpy(), seg[2].cpu().numpy()),
                                    second_half, f"kernel {kernel}, second segmented launch")
    # two families, two layouts: the records concatenate
    first, second = case.offered[0], case.offered[-1]
    assert first != second, f"shape {shape_index} offers one family only: {case.offered}"
    waves_a, waves_b = base._waves_offered(case, first), base._waves_offered(case, second)
    pairs = [(x, y) for x in waves_a for y in reversed(waves_b) if x != y]
    assert pairs, f"{first} offers {waves_a}, {second} offers {waves_b}: no two different layouts"
    wa, wb = pairs[0]
    state = case.net.new_state(base.B)
    rec_a = _one_launch(case, first, wa, 0, cut, S, state, True)[5]
    rec_b = _one_launch(case, second, wb, cut, base.T, S, state, True)[5]
    one = _one_launch(case, first, 0, 0, base.T, S, case.net.new_state(base.B), True)[5]
    both = torch.cat([rec_a, rec_b], dim=1)
    assert tuple(one.shape) == (base.B, base.T // S, len(case.res.out_idx), 4) and one.dtype == torch.int32
    assert torch.equal(both, one), f"{first} ({wa} waves) then {second} ({wb} waves): records against one launch"
    for K, H in ((1, 1), (3, 1)):                              # windows over the concatenation straddle the launches
        got = case.net.segment_features(both, S, ALL_KEYS, K, H).cpu().numpy()
        np.testing.assert_array_equal(got, _ref_rows(case, S, K, H), err_msg=f"records of two launches, K={K}")


def test_dense_kernel_both_record_forms(torch_cuda, oracle_c):
    """lif_dense.h keeps the records in registers up to 4 slots per lane (FEATREG) and in LDS above; `plan()` reports the
    slots.  Expected: N = 256 at 4 waves per clip -> 1 slot (registers); N = 2048 at 2 waves -> 16 slots, N = 1024 at 1
    wave -> 16 slots (LDS).  Every (shape, waves) the dense kernel offers is planned, one of each form runs."""
    from lsm_speech_classifier_amd import _lib
    base = _base()
    S = 24
    found = {}
    for shape_index in (0, 3, 1):
        case = _case(oracle_c, shape_index)
        if "dense" not in case.offered:
            continue
        for wpc in (1, 2, 4, 8, 16):
            case.net.set_kernel("dense")
            try:
                plan = case.net.plan(base.B, base.T, wpc)
            except _lib.LsmHipError:
                continue
            finally:
                case.net.set_kernel("auto")
            assert plan["kernel"] == "dense" and plan["waves_per_clip"] == wpc
            form = "registers" if plan["slots_per_lane"] <= 4 else "lds"
            found.setdefault(form, (shape_index, wpc, plan["slots_per_lane"]))
    print("dense record forms:", found)
    assert set(found) == {"registers", "lds"}, f"dense layouts planned: {found}"
    for form, (shape_index, wpc, slots) in found.items():
        case = _case(oracle_c, shape_index)
        got = _run(case, "dense", S, ALL_KEYS, wpc=wpc).cpu().numpy()
        np.testing.assert_array_equal(got, _ref_rows(case, S), err_msg=f"dense, records in {form} ({slots} slots, {wpc} waves)")
        whole = _run(case, "dense", 8, ALL_KEYS, K=base.T // 8, wpc=wpc).cpu().numpy()[:, 0]
        np.testing.assert_array_equal(whole, np.stack([row[0] for row in case.ref[tuple(ALL_KEYS)]]))
        _DENSE_FORMS.add(form)


def test_refusals_launch_nothing(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    base = _base()
    case = _case(oracle_c, 0)
    net, n_out = case.net, len(case.res.out_idx)
    r = torch.from_numpy(case.rasters).cuda()
    keys = np.arange(8, dtype=np.int32)
    SENT = 0x5A5A5A5A
    rec = torch.full((base.B, base.T, n_out, 4), SENT, dtype=torch.int32, device="cuda")      # room for S = 1
    feats = torch.full((base.B, base.T, 8 * n_out), -7.0, dtype=torch.float32, device="cuda")
    state = net.new_state(base.B)
    stream = torch.cuda.current_stream().cuda_stream

    def run(S, n_steps=base.T, first=0, st_in=None, records=rec.data_ptr()):
        return net.lib.lsm_reservoir_run_segments(
            net._handle, C.c_void_p(r.data_ptr()), base.B, n_steps, S, first, st_in, None,
            C.c_void_p(records) if records else None, C.c_void_p(keys.ctypes.data), 8, C.c_void_p(feats.data_ptr()),
            None, None, None, 0, None, 0, stream)

    def windows(G, S, K, H, records=rec.data_ptr()):
        return net.lib.lsm_segment_features(net._handle, C.c_void_p(records), base.B, G, S, K, H,
                                            C.c_void_p(keys.ctypes.data), 8, C.c_void_p(feats.data_ptr()), stream)

    refused = [
        (run(0), "segment_steps"), (run(-3), "segment_steps"), (run(36), "multiple"), (run(25), "multiple"),
        (run(24, records=rec.data_ptr() + 4), "aligned"), (run(24, records=0), "records_out"),
        (run(24, first=5), "first_step"), (run(24, first=-1), "first_step"), (run(24, first=65535 - 24), "first_step"),
        (run(24, st_in=C.c_void_p(state.data.data_ptr() + 4)), "state_in"),
        (windows(4, 0, 1, 1), "segment_steps"), (windows(4, 24, 0, 1), "window_segments"),
        (windows(4, 24, 5, 1), "window_segments"), (windows(4, 24, 1, 0), "hop_segments"),
        (windows(4, 24, 1, -1), "hop_segments"), (windows(96, 700, 94, 1), "65535"),
        (windows(4, 24, 1, 1, records=rec.data_ptr() + 8), "aligned"),
    ]
    for i, (rc, word) in enumerate(refused):
        assert rc == -1, f"refusal {i} ({word}): returned {rc}"
    # the reason of each, through the Python layer's error (one call each: lsm_last_error holds the latest)
    for call, word in ((lambda: run(0), "segment_steps"), (lambda: run(36), "multiple"),
                       (lambda: run(24, records=rec.data_ptr() + 4), "aligned"), (lambda: run(24, first=5), "first_step"),
                       (lambda: windows(4, 24, 5, 1), "window_segments"), (lambda: windows(4, 24, 1, 0), "hop_segments"),
                       (lambda: windows(96, 700, 94, 1), "65535")):
        with pytest.raises(_lib.LsmHipError, match=word):
            _lib.check(call(), "refused")
    torch.cuda.synchronize()
    assert bool((rec == SENT).all()) and bool((feats == -7.0).all()), "a refused call wrote to its outputs"
    # the Python layer refuses before it launches
    for kw in (dict(segment_steps=36), dict(segment_steps=0), dict(segment_steps=24, window_segments=5),
               dict(segment_steps=24, hop_segments=0)):
        with pytest.raises(_lib.LsmHipError):
            net.run_segments(r, **kw)
    # 65535 steps per window is the last accepted: 3 segments of 21845 steps; the handle still works
    assert windows(4, 21845, 3, 1) == 0 and windows(4, 21846, 3, 1) == -1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(net.run_segments(r, 24, ALL_KEYS).cpu().numpy(), _ref_rows(case, 24))


def test_sliding_windows_over_a_recording(torch_cuda, oracle_c):
    """2 recordings of 3 audio windows, 16 gammatone filters, N = 256: windows of K = 4 segments of S = 100 steps, hop 1,
    against the oracle run over the concatenated rasters, sliced (windows straddle the audio windows)."""
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
    n_rec, windows, S, K, H = 2, 3, 100, 4, 1
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    steps = fe.n_steps
    assert steps * windows == 1200
    res = R.build_reservoir(R.SimulationParams(num_neurons=256, num_output_neurons=100, small_world_graph_k=50,
                                               mean_weight=2.0 / 25, refractory_period=2), fe.n_channels)
    net = snn.SNN(None, reservoir=res)
    clips = synth.class_chirps([0, 5, 9, 3, 7, 11], seed=31)
    audio = np.ascontiguousarray(clips.reshape(n_rec, windows * clips.shape[1]))
    rasters = fe.encode(torch.from_numpy(clips).cuda()).cpu().numpy().reshape(n_rec, windows, fe.n_channels, steps)
    whole = np.concatenate([rasters[:, w] for w in range(windows)], axis=2)      # (n_rec, C, 1200)
    got = pipeline.sliding_features_from_long_audio(audio, fe, net, ALL_KEYS, S, K, H).cpu().numpy()
    G = 1200 // S
    assert got.shape == (n_rec, G - K + 1, 8 * 100)
    for i in range(n_rec):
        sm = oracle_c.lif_run(res, whole[i], ALL_KEYS)[1]
        assert sm[:, res.out_idx].any()
        for w in range(G - K + 1):
            want = ref_numpy.feature_row(sm[w * H * S:(w * H + K) * S], res.out_idx, int(res.burst_isi_max), ALL_KEYS)
            np.testing.assert_array_equal(got[i, w], want, err_msg=f"recording {i}, window {w}")
    two = pipeline.sliding_features_from_long_audio(audio, fe, net, TWO_KEYS, 200, 2, 3).cpu().numpy()
    assert two.shape == (n_rec, (6 - 2) // 3 + 1, 2 * 100)
    sm = oracle_c.lif_run(res, whole[1], ALL_KEYS)[1]
    np.testing.assert_array_equal(two[1, 1], ref_numpy.feature_row(sm[600:1000], res.out_idx, int(res.burst_isi_max), TWO_KEYS))


def test_hot_path_time_segments(torch_cuda):
    """HotPath(time_segments=4) rows are run_segments' rows side by side; HotPath() rows are run_batch's (today's)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    res = R.build_reservoir(R.SimulationParams(num_neurons=256, num_output_neurons=100, small_world_graph_k=50,
                                               mean_weight=2.0 / 25, refractory_period=2), fe.n_channels)
    net = snn.SNN(None, reservoir=res)
    audio = torch.from_numpy(synth.class_chirps([0, 5, 9, 3, 7, 11, 2], seed=5)).cuda()
    rasters = fe.encode(audio)
    T = fe.n_steps
    assert T % 4 == 0
    want4 = net.run_segments(rasters, T // 4, ALL_KEYS).reshape(len(audio), -1)
    want1 = net.run_batch(rasters, ALL_KEYS)[0]
    assert want4.shape[1] == 4 * want1.shape[1] and bool(want4.any())
    for streams in (1, 3):
        hp4 = pipeline.HotPath(fe, net, ALL_KEYS, streams=streams, time_segments=4)
        got4 = hp4.run([audio[:4], audio[4:]])
        assert torch.equal(got4, want4), f"{streams} streams: time_segments=4 against run_segments"
        out = torch.zeros_like(want4)
        stats = torch.zeros((len(audio), 2), dtype=torch.int32, device="cuda")
        hp4.submit(audio, stats_out=stats, out=out)
        hp4.synchronize()
        assert torch.equal(out, want4) and bool(stats.any())
        got1 = pipeline.HotPath(fe, net, ALL_KEYS, streams=streams).run([audio[:4], audio[4:]])
        assert torch.equal(got1, want1), f"{streams} streams: the default pipeline against run_batch"
    via = pipeline.features_from_audio(audio.cpu().numpy(), fe, net, ALL_KEYS, batch=4, time_segments=4)
    np.testing.assert_array_equal(via, want4.cpu().numpy())
    with pytest.raises(ValueError, match="time_segments"):
        pipeline.HotPath(fe, net, ALL_KEYS, time_segments=7)


def test_cfg2_size_against_the_oracle(torch_cuda, oracle_c):
    """N = 1000, 128 channels, T = 400, B = 256, S = 100: the per-segment rows of a handful of clips of the batch."""
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import reservoir as R, snn
    n, c, t, b, S = 1000, 128, 400, 256, 100
    res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=400, small_world_graph_k=200,
                                               mean_weight=2.0 / 100, refractory_period=2), c)
    rasters = (np.random.RandomState(2).random_sample((b, c, t)) < 0.1).astype(np.uint8)
    net = snn.SNN(None, reservoir=res)
    got, rec = net.run_segments(torch.from_numpy(rasters).cuda(), S, ALL_KEYS, want_records=True)
    assert tuple(got.shape) == (b, t // S, 8 * 400) and tuple(rec.shape) == (b, t // S, 400, 4)
    plain = net.run_batch(rasters, ALL_KEYS)[0]
    assert torch.equal(net.segment_features(rec, S, ALL_KEYS, t // S, 1)[:, 0], plain)
    got = got.cpu().numpy()
    for i in (0, 1, 100, 255):
        whole, sm, _ = oracle_c.lif_run(res, rasters[i], ALL_KEYS)
        assert sm[:, res.out_idx].any()
        np.testing.assert_array_equal(plain[i].cpu().numpy(), whole, err_msg=f"clip {i}: run_batch against the oracle")
        for g in range(t // S):
            want = ref_numpy.feature_row(sm[g * S:(g + 1) * S], res.out_idx, int(res.burst_isi_max), ALL_KEYS)
            np.testing.assert_array_equal(got[i, g], want, err_msg=f"clip {i}, segment {g}")


def test_every_family_ran_segmented(torch_cuda):
    """Last in the module: every kernel family ran a segmented launch, the dense kernel with both record forms."""
    base = _base()
    missing = [kernel for kernel in base.KERNELS if kernel not in _RAN]
    assert not missing, f"kernel families that never ran a segmented launch: {missing} (ran: {sorted(_RAN)})"
    assert _DENSE_FORMS == {"registers", "lds"}, f"dense record forms that ran: {sorted(_DENSE_FORMS)}"
