"""Open-ended streams (SPEC.md 4d, include/lsm_hip_streams.h: `lsm_reservoir_run_stream`, `lsm_segment_features_ragged`,
`SNN.run_stream_records`, `SNN.segment_features(segments=)`, `pipeline.StreamBank`,
`pipeline.sliding_features_from_recordings`).

Every comparison is exact.  The reference is the plain-C oracle's spike matrix of the WHOLE uncut run (the cached cases of
tests/test_gpu_state.py: four reservoirs, T = 96, B = 3), sliced on the host and turned into rows by the oracle's own
`spike_features` (tests/test_gpu_segments.py::_ref_rows); the code under test is never its own reference.  Every kernel
family a reservoir offers runs; the last test of the module fails when one of them never ran a stream launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
TWO_KEYS = ['burst_counts', 'spike_variances']              # a subset, not in the default order
FILL = 0x5A
FILL32 = 0x5A5A5A5A
CUT = 72                                                    # a cut through activity and a boundary of S = 8 and S = 24
_RAN = set()                                                # kernel families that ran at least one stream launch


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


def _seg():
    import test_gpu_segments as seg                         # _case (with the oracle's preconditions), _ref_rows
    return seg


def _shape_ids():
    return [f"N{n}-C{c}" for n, _, _, c in [(256, 50, 100, 40), (1024, 204, 410, 64), (1024, 204, 410, 160),
                                            (2048, 408, 820, 128)]]


def _filled(torch, shape, dtype):
    """A device tensor whose every byte is 0x5A."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def _bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _feat_offset(n_neurons):
    np_ = (n_neurons + 63) // 64 * 64
    return 16 + 6 * np_ + np_ // 4


def _raw_stream(case, kernel, rasters, S, segs, state_in, longest_first):
    """One lsm_reservoir_run_stream call through ctypes into outputs pre-filled with 0x5A, out of place.  Returns
    (records, spike matrix, trace, statistics, state_out) as device tensors."""
    import torch
    net = case.net
    net.set_kernel(kernel)
    _RAN.add(kernel)
    try:
        r = torch.from_numpy(np.ascontiguousarray(rasters)).cuda()
        n, _, T = r.shape
        n_out, N = len(case.res.out_idx), case.res.num_neurons
        rec = _filled(torch, (n, T // S, n_out, 4), torch.int32)
        sm = _filled(torch, (n, T, N), torch.uint8)
        vt = _filled(torch, (n, T, N), torch.float32)
        stats = _filled(torch, (n, 2), torch.int32)
        out = _filled(torch, (n, net.state_bytes()), torch.uint8)
        counts = torch.tensor(list(segs), dtype=torch.int32, device="cuda")
        need = net.lib.lsm_reservoir_order_workspace(n) if longest_first else 0
        ws = torch.empty((need + 3) // 4, dtype=torch.int32, device="cuda") if longest_first else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = net.lib.lsm_reservoir_run_stream(net._handle, p(r), n, T, S, p(counts), p(state_in), p(out), p(rec), p(sm), p(vt),
                                              p(stats), 0, p(ws), need, torch.cuda.current_stream().cuda_stream)
        from lsm_speech_classifier_amd import _lib
        _lib.check(rc, "lsm_reservoir_run_stream")
        torch.cuda.synchronize()
        return rec, sm, vt, stats, out
    finally:
        net.set_kernel("auto")


# ------------------------------------------------------------------------------- tests ----
RAGGED = [(8, (12, 5, 0)), (8, (1, 12, 7)), (24, (4, 1, 0)), (24, (2, 4, 3)), (1, (96, 37, 0)), (96, (1, 0, 1))]


@pytest.mark.parametrize("S,segs", RAGGED, ids=[f"S{S}-{'_'.join(map(str, g))}" for S, g in RAGGED])
@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_ragged_records(torch_cuda, oracle_c, shape_index, S, segs):
    """One launch from reset, per-clip segment counts: what a clip ran equals the oracle, everything behind it keeps the
    fill, a clip of 0 segments is not touched and its state block passes through."""
    torch = torch_cuda
    base, seg = _base(), _seg()
    assert _shape_ids() == base.SHAPE_IDS and base.T == 96 and base.B == 3
    case = seg._case(oracle_c, shape_index)
    net, n_out = case.net, len(case.res.out_idx)
    G = base.T // S
    ref = case.ref[tuple(ALL_KEYS)]
    want = {tuple(keys): seg._ref_rows(case, S, keys=keys) for keys in (ALL_KEYS, TWO_KEYS)}
    state_in = torch.zeros((base.B, net.state_bytes()), dtype=torch.uint8, device="cuda")
    for b, g in enumerate(segs):
        if g == 0:
            state_in[b] = 0x3C                              # a block the launch must hand on byte for byte
    for kernel in case.offered:
        outs = {}
        for longest_first in (False, True):
            rec, sm, vt, stats, out = _raw_stream(case, kernel, case.rasters, S, segs, state_in, longest_first)
            outs[longest_first] = [_bytes(x) for x in (rec, sm, vt, stats, out)]
            msg = f"kernel {kernel}, S={S}, segments {segs}, longest_first={longest_first}"
            rec_h, sm_h, vt_h = rec.cpu().numpy(), sm.cpu().numpy(), vt.cpu().numpy()
            for b, g in enumerate(segs):
                L = g * S
                assert (rec_h[b, g:].view(np.uint32) == FILL32).all(), f"records behind clip {b}'s segments, {msg}"
                assert (sm_h[b, L:] == FILL).all(), f"spike-matrix rows behind clip {b}'s steps, {msg}"
                assert (vt_h[b, L:].view(np.uint32) == FILL32).all(), f"trace rows behind clip {b}'s steps, {msg}"
                np.testing.assert_array_equal(sm_h[b, :L], ref[b][1][:L], err_msg=f"spike matrix, clip {b}, {msg}")
                np.testing.assert_array_equal(vt_h[b, :L], ref[b][2][:L], err_msg=f"membrane trace, clip {b}, {msg}")
                if g == 0:
                    assert (stats[b].cpu().numpy().view(np.uint32) == FILL32).all(), f"statistics of idle clip {b}, {msg}"
                    assert torch.equal(out[b], state_in[b]), f"state block of idle clip {b}, {msg}"
                else:
                    per = ref[b][1][:L].sum(axis=0, dtype=np.int64)
                    assert stats[b].tolist() == [int(np.count_nonzero(per)), int(per.sum())], f"statistics, clip {b}, {msg}"
                    assert not out[b, _feat_offset(case.res.num_neurons):].any(), f"feat block of clip {b}, {msg}"
            counts = np.asarray(segs)
            for keys in (ALL_KEYS, TWO_KEYS):
                rows = _filled(torch, (base.B, G, len(keys) * n_out), torch.float32)
                got = net.segment_features(rec, S, keys, 1, 1, features_out=rows, segments=counts)
                assert got is rows
                rows_h = rows.cpu().numpy()
                for b, g in enumerate(segs):
                    np.testing.assert_array_equal(rows_h[b, :g], want[tuple(keys)][b, :g],
                                                  err_msg=f"rows, clip {b}, {len(keys)} keys, {msg}")
                    assert (rows_h[b, g:].view(np.uint32) == FILL32).all(), f"rows behind clip {b}'s segments, {msg}"
                # the counts as a device tensor, into a tensor allocated by the call: unwritten rows read as zeros
                dev = net.segment_features(rec, S, keys, 1, 1, segments=torch.tensor(segs, dtype=torch.int32, device="cuda"))
                for b, g in enumerate(segs):
                    np.testing.assert_array_equal(dev[b, :g].cpu().numpy(), want[tuple(keys)][b, :g])
                    assert not dev[b, g:].any()
        for a, b_ in zip(outs[False], outs[True]):
            assert np.array_equal(a, b_), f"kernel {kernel}, S={S}, segments {segs}: the two start orders differ"


def test_ragged_records_of_more_clips_than_compute_units(torch_cuda, oracle_c):
    """More clips than compute units: the longest-first start really ranks the clips by their input inside their own
    segments (`clip_keys_ragged_kernel`), and gives the bytes of the plain order."""
    torch = torch_cuda
    base, seg = _base(), _seg()
    case = seg._case(oracle_c, 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = cus // base.B + 1
    many = np.ascontiguousarray(np.tile(case.rasters, (reps, 1, 1)))
    S = 8
    segs = [(5 * i + 3) % 13 for i in range(len(many))]                 # 0 .. 12, zeros included
    assert len(many) > cus and 0 in segs and 12 in segs
    want = seg._ref_rows(case, S)
    state_in = torch.zeros((len(many), case.net.state_bytes()), dtype=torch.uint8, device="cuda")
    for kernel in case.offered:
        plain = _raw_stream(case, kernel, many, S, segs, state_in, False)
        ordered = _raw_stream(case, kernel, many, S, segs, state_in, True)
        for a, b_ in zip(plain, ordered):
            assert torch.equal(a, b_), f"kernel {kernel}: the two start orders differ"
        rows = case.net.segment_features(ordered[0], S, ALL_KEYS, segments=np.asarray(segs)).cpu().numpy()
        for i, g in enumerate(segs):
            np.testing.assert_array_equal(rows[i, :g], want[i % base.B, :g], err_msg=f"kernel {kernel}, clip {i}")
            assert not rows[i, g:].any()


@pytest.mark.parametrize("S,K,H", [(8, 3, 2), (24, 2, 1)])
@pytest.mark.parametrize("shape_index", range(4), ids=_shape_ids())
def test_streams_at_different_positions_share_a_launch(torch_cuda, oracle_c, shape_index, S, K, H):
    """Launch 1: clip 0 runs all 96 steps, clip 1 its first 72, clip 2 nothing.  Launch 2: clip 0 nothing, clip 1 its steps
    72..95 at columns 0..23, clip 2 all 96 -- from a state whose feat block holds garbage."""
    torch = torch_cuda
    base, seg = _base(), _seg()
    case = seg._case(oracle_c, shape_index)
    net, res = case.net, case.res
    ref = case.ref[tuple(ALL_KEYS)]
    T, G = base.T, base.T // S
    # the precondition, on the oracle: the cut goes through activity in every clip and is a segment boundary
    assert CUT % S == 0 and T % S == 0
    for b in range(base.B):
        assert base._cut_is_through_activity(ref[b][1], res, CUT), f"step {CUT} is no cut through activity for clip {b}"
    first = case.rasters
    second = np.ones_like(first)                                        # what lies behind a clip's steps influences nothing
    second[1, :, :T - CUT] = first[1, :, CUT:]
    second[2] = first[2]
    segs1, segs2 = (G, CUT // S, 0), (0, (T - CUT) // S, G)
    want1 = seg._ref_rows(case, S)
    wantK = seg._ref_rows(case, S, K, H)
    off = _feat_offset(res.num_neurons)
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        try:
            state = net.new_state(base.B)
            stats = torch.full((base.B, 2), -1, dtype=torch.int32, device="cuda")
            rec1, sm1, vt1 = net.run_stream_records(first, S, segs1, state=state, want_spike_matrix=True, want_v_trace=True,
                                                    stats_out=stats)
            assert state.steps_done == 0 and not state.ended.any()
            assert not state.data[:, off:].any(), f"kernel {kernel}: feat block after launch 1"
            state.data[:, off:] = 0xEE                                  # garbage: launch 2 must not read it
            rec2, sm2, vt2 = net.run_stream_records(second, S, segs2, state=state, want_spike_matrix=True,
                                                    want_v_trace=True, stats_out=stats)
            assert state.steps_done == 0 and not state.ended.any()
        finally:
            net.set_kernel("auto")
        msg = f"kernel {kernel}, S={S}"
        records = torch.stack([rec1[0], torch.cat([rec1[1, :CUT // S], rec2[1, :(T - CUT) // S]]), rec2[2]])
        np.testing.assert_array_equal(net.segment_features(records, S, ALL_KEYS).cpu().numpy(), want1, err_msg=msg)
        np.testing.assert_array_equal(net.segment_features(records, S, ALL_KEYS, K, H).cpu().numpy(), wantK,
                                      err_msg=f"{msg}, windows K={K} H={H}")
        sm = torch.stack([sm1[0], torch.cat([sm1[1, :CUT], sm2[1, :T - CUT]]), sm2[2]]).cpu().numpy()
        vt = torch.stack([vt1[0], torch.cat([vt1[1, :CUT], vt2[1, :T - CUT]]), vt2[2]]).cpu().numpy()
        assert not sm2[0].any() and not sm1[2].any() and not sm2[1, T - CUT:].any()      # rows nobody ran stay zeros
        # the state of every clip after its step 95
        v, rf, last = state.membrane().cpu().numpy(), state.refractory().cpu().numpy(), state.last_spikes().cpu().numpy()
        ever, total = state.ever_fired().cpu().numpy(), state.spike_total().cpu().numpy()
        # clip 0 stopped after launch 1 and passed through launch 2 in place: only its feat block was overwritten above
        feat = state.data[:, off:].cpu().numpy()
        assert (feat[0] == 0xEE).all() and not feat[1:].any(), f"{msg}: feat blocks"
        for b in range(base.B):
            sm_ref, vt_ref = ref[b][1], ref[b][2]
            np.testing.assert_array_equal(sm[b], sm_ref, err_msg=f"spike matrix, clip {b}, {msg}")
            np.testing.assert_array_equal(vt[b], vt_ref, err_msg=f"membrane trace, clip {b}, {msg}")
            np.testing.assert_array_equal(v[b], vt_ref[T - 1], err_msg=f"membrane, clip {b}, {msg}")
            np.testing.assert_array_equal(rf[b], base._refractory_after(sm_ref, T - 1, int(res.refractory_period)),
                                          err_msg=f"refractory, clip {b}, {msg}")
            np.testing.assert_array_equal(last[b], sm_ref[T - 1].astype(bool), err_msg=f"last spikes, clip {b}, {msg}")
            np.testing.assert_array_equal(ever[b], sm_ref.any(axis=0), err_msg=f"ever fired, clip {b}, {msg}")
            assert int(total[b]) == int(sm_ref.sum(dtype=np.int64)), f"spike total, clip {b}, {msg}"
            assert stats[b].tolist() == ref[b][3], f"statistics, clip {b}, {msg}"


def test_a_stream_runs_past_65535_steps(torch_cuda, oracle_c):
    """70 000 steps in launches of max_steps: rows of segments behind step 65 535 and a window that straddles it equal the
    oracle's, where every bounded entry refuses."""
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import _lib
    base, seg = _base(), _seg()
    case = seg._case(oracle_c, 0)
    net, res = case.net, case.res
    assert (res.num_neurons, res.n_channels) == (256, 40)
    S, n_steps, n_streams = 500, 70000, 2
    G = n_steps // S
    stop = [G, 101]                                                     # stream 1 stops after segment 100
    rasters = np.stack([(np.random.RandomState(7 + b).random_sample((40, n_steps)) < 0.35).astype(np.uint8)
                        for b in range(n_streams)])
    sm = oracle_c.lif_run(res, rasters[0], ALL_KEYS)[1]
    so = sm[:, res.out_idx]
    assert all(so[g * S:(g + 1) * S].any() for g in range(131, G)), "a segment behind step 65535 without output spikes"
    burst = int(res.burst_isi_max)

    def ref_row(matrix, a, e):
        return ref_numpy.feature_row(matrix[a:e], res.out_idx, burst, ALL_KEYS)

    chunk = net.max_steps(n_streams) // S * S
    assert S <= chunk < 65535
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        try:
            state = net.new_state(n_streams)
            stats = torch.full((n_streams, 2), -1, dtype=torch.int32, device="cuda")
            r = torch.from_numpy(rasters).cuda()
            recs = []
            for t0 in range(0, n_steps, chunk):
                n = min(chunk, n_steps - t0)
                segs = [min(max(g - t0 // S, 0), n // S) for g in stop]
                recs.append((segs, net.run_stream_records(r[:, :, t0:t0 + n], S, segs, state=state, stats_out=stats)[0]))
            assert len(recs) >= 2 and any(0 < s[1] < len(x[1]) for s, x in recs)      # stream 1 ended inside a launch
            per_stream = [torch.cat([x[b, :s[b]] for s, x in recs]) for b in range(n_streams)]
            assert [len(p) for p in per_stream] == stop
            records = torch.zeros((n_streams, G) + tuple(per_stream[0].shape[1:]), dtype=torch.int32, device="cuda")
            for b in range(n_streams):
                records[b, :stop[b]] = per_stream[b]
            rows = net.segment_features(records, S, ALL_KEYS, segments=np.asarray(stop)).cpu().numpy()
            for g in range(128, G):
                np.testing.assert_array_equal(rows[0, g], ref_row(sm, g * S, (g + 1) * S), err_msg=f"{kernel}: segment {g}")
            pairs = net.segment_features(records, S, ALL_KEYS, 2, 1, segments=np.asarray(stop)).cpu().numpy()
            assert 130 * S < 65535 < 132 * S
            np.testing.assert_array_equal(pairs[0, 130], ref_row(sm, 130 * S, 132 * S), err_msg=f"{kernel}: window 130-131")
            per = sm.sum(axis=0, dtype=np.int64)
            assert int(per.sum()) < 2 ** 31
            assert stats[0].tolist() == [int(np.count_nonzero(per)), int(per.sum())], f"{kernel}: statistics of stream 0"
            assert int(state.spike_total()[0]) == int(per.sum())
            # the bounded entries still refuse this position
            bounded = net.new_state(n_streams)
            bounded.steps_done = 65000
            with pytest.raises(_lib.LsmHipError, match="first_step"):
                net.run_segment_records(r[:, :, 65000:66000], S, state=bounded)
        finally:
            net.set_kernel("auto")
    # stream 1, which stopped earlier and rode along with 0 segments: its last rows, against the oracle over its own steps
    sm1 = oracle_c.lif_run(res, np.ascontiguousarray(rasters[1][:, :stop[1] * S]), ALL_KEYS)[1]
    for g in range(stop[1] - 3, stop[1]):
        np.testing.assert_array_equal(rows[1, g], ref_row(sm1, g * S, (g + 1) * S), err_msg=f"stream 1, segment {g}")
    assert not rows[1, stop[1]:].any()
    per1 = sm1.sum(axis=0, dtype=np.int64)
    assert stats[1].tolist() == [int(np.count_nonzero(per1)), int(per1.sum())]


def test_stream_bank(torch_cuda, oracle_c):
    torch = torch_cuda
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import pipeline
    base, seg = _base(), _seg()
    case = seg._case(oracle_c, 1)
    net, res = case.net, case.res
    S, K, H = 8, 3, 2
    pushes = [(4, 0, 1), (0, 3, 5), (8, 9, 0), (0, 0, 6)]
    assert np.sum(pushes, axis=0).tolist() == [base.T // S] * 3
    want = seg._ref_rows(case, S, K, H)
    fresh = (np.random.RandomState(4242).random_sample((res.n_channels, base.T)) < base.DENSITY).astype(np.uint8)
    sm_fresh = oracle_c.lif_run(res, fresh, ALL_KEYS)[1]
    assert sm_fresh[:, res.out_idx].any()
    want_fresh = np.stack([ref_numpy.feature_row(sm_fresh[w * H * S:(w * H + K) * S], res.out_idx, int(res.burst_isi_max),
                                                 ALL_KEYS) for w in range((base.T // S - K) // H + 1)])
    for kernel in case.offered:
        net.set_kernel(kernel)
        _RAN.add(kernel)
        try:
            bank = pipeline.StreamBank(net, 3, S, K, H, ALL_KEYS)
            seen = np.zeros(3, dtype=np.int64)
            got = [[] for _ in range(3)]
            for new in pushes:
                g_max = max(new)
                push = np.ones((3, res.n_channels, g_max * S), dtype=np.uint8)       # behind a stream's steps: ignored
                for b, g in enumerate(new):
                    push[b, :, :g * S] = case.rasters[b][:, seen[b] * S:(seen[b] + g) * S]
                rows, counts = bank.push(push, new)
                plan = [pipeline.stream_window_plan(int(seen[b]), int(new[b]), K, H)[0] for b in range(3)]
                assert counts.tolist() == plan, f"{kernel}: counts of push {new}"
                assert rows.shape[0] == 3 and rows.shape[1] >= max(plan)
                for b in range(3):
                    got[b].append(rows[b, :plan[b]].cpu().numpy())
                    assert not rows[b, plan[b]:].any()
                seen += np.asarray(new)
            for b in range(3):
                np.testing.assert_array_equal(np.concatenate(got[b]), want[b], err_msg=f"{kernel}: stream {b}")
            # a stream ends, a new one takes its slot
            before = bank.state.data.clone()
            bank.reset([1])
            assert bank.seen.tolist() == [12, 0, 12] and not bank.state.data[1].any()
            push = np.zeros((3, res.n_channels, base.T), dtype=np.uint8)
            push[1] = fresh
            rows, counts = bank.push(push, (0, 12, 0))
            assert counts.tolist() == [0, len(want_fresh), 0]
            np.testing.assert_array_equal(rows[1, :counts[1]].cpu().numpy(), want_fresh, err_msg=f"{kernel}: the new stream")
            assert not rows[0].any() and not rows[2].any()
            assert torch.equal(bank.state.data[0], before[0]) and torch.equal(bank.state.data[2], before[2])
            assert bank.seen.tolist() == [12, 12, 12]
        finally:
            net.set_kernel("auto")


def test_sliding_features_from_recordings(torch_cuda):
    """Recordings of 1, 3 and 2 audio windows in one batch: each one's rows are those of
    `sliding_features_from_long_audio` on that recording alone (pinned to the oracle by tests/test_gpu_segments.py)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, frontend, pipeline, reservoir as R, snn, synth
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    res = R.build_reservoir(R.SimulationParams(num_neurons=256, num_output_neurons=100, small_world_graph_k=50,
                                               mean_weight=2.0 / 25, refractory_period=2), fe.n_channels)
    net = snn.SNN(None, reservoir=res)
    clips = synth.class_chirps([0, 5, 9, 3, 7, 11], seed=31)
    windows = [1, 3, 2]
    bounds = np.concatenate([[0], np.cumsum(windows)])
    recordings = [np.ascontiguousarray(clips[bounds[i]:bounds[i + 1]].reshape(-1)) for i in range(3)]
    S, K, H = 100, 4, 1
    Gt = fe.n_steps // S
    assert fe.n_steps % S == 0 and Gt >= K
    ran = 0
    for kernel in _base().KERNELS:
        try:
            net.set_kernel(kernel)
        except _lib.LsmHipError:
            continue
        ran += 1
        _RAN.add(kernel)
        for keys, (s, k, h) in ((ALL_KEYS, (S, K, H)), (TWO_KEYS, (2 * S, 2, 3))):
            rows, counts = pipeline.sliding_features_from_recordings(recordings, fe, net, keys, s, k, h)
            gt = fe.n_steps // s
            assert counts.tolist() == [(w * gt - k) // h + 1 for w in windows]
            assert tuple(rows.shape) == (3, max(counts), len(keys) * 100)
            for i, rec in enumerate(recordings):
                alone = pipeline.sliding_features_from_long_audio(rec[None], fe, net, keys, s, k, h)
                assert alone.shape[1] == counts[i] and bool(alone.any())
                assert torch.equal(rows[i, :counts[i]], alone[0]), f"{kernel}: recording {i}"
                assert not rows[i, counts[i]:].any(), f"{kernel}: rows past recording {i}'s count"
    assert ran
    net.set_kernel("auto")


def test_refusals_launch_nothing(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    base, seg = _base(), _seg()
    case = seg._case(oracle_c, 0)
    net, n_out = case.net, len(case.res.out_idx)
    r = torch.from_numpy(case.rasters).cuda()
    keys = np.arange(8, dtype=np.int32)
    rec = torch.full((base.B, base.T, n_out, 4), FILL32, dtype=torch.int32, device="cuda")      # room for S = 1
    feats = torch.full((base.B, base.T, 8 * n_out), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((base.B + 1,), 2, dtype=torch.int32, device="cuda")
    odd = C.c_void_p(counts.view(torch.uint8)[2:].data_ptr())
    state = net.new_state(base.B)
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda x: C.c_void_p(x) if x else None

    def run(S, n_steps=base.T, segs=None, st_in=None, st_out=None, records=rec.data_ptr(), wpc=0, n_clips=base.B):
        return net.lib.lsm_reservoir_run_stream(net._handle, C.c_void_p(r.data_ptr()), n_clips, n_steps, S, segs, st_in, st_out,
                                                void(records), None, None, None, wpc, None, 0, stream)

    def windows(G, S, K, H, records=rec.data_ptr(), segs=C.c_void_p(counts.data_ptr()), n_keys=8):
        return net.lib.lsm_segment_features_ragged(net._handle, void(records), base.B, G, segs, S, K, H,
                                                   C.c_void_p(keys.ctypes.data), n_keys, C.c_void_p(feats.data_ptr()), stream)

    misaligned = C.c_void_p(state.data.data_ptr() + 4)
    cases = [
        (lambda: run(0), "segment_steps"), (lambda: run(-3), "segment_steps"), (lambda: run(36), "segment_steps"),
        (lambda: run(25), "segment_steps"), (lambda: run(24, records=0), "records_out"),
        (lambda: run(24, records=rec.data_ptr() + 4), "records_out"), (lambda: run(24, segs=odd), "clip_segments"),
        (lambda: run(24, st_in=misaligned), "state_in"), (lambda: run(24, st_out=misaligned), "state_out"),
        (lambda: run(24, wpc=17), "waves_per_clip"), (lambda: run(1, n_steps=0), "n_steps"),
        (lambda: run(1, n_steps=65536), "n_steps"), (lambda: run(24, n_clips=-1), "n_clips"),
        (lambda: windows(4, 24, 1, 1, segs=None), "clip_segments"), (lambda: windows(4, 24, 1, 1, segs=odd), "clip_segments"),
        (lambda: windows(96, 700, 94, 1), "65535"), (lambda: windows(4, 0, 1, 1), "segment_steps"),
        (lambda: windows(4, 24, 0, 1), "window_segments"), (lambda: windows(4, 24, 5, 1), "window_segments"),
        (lambda: windows(4, 24, 1, 0), "hop_segments"), (lambda: windows(4, 24, 1, 1, records=rec.data_ptr() + 8), "records"),
        (lambda: windows(4, 24, 1, 1, n_keys=0), "n_keys"), (lambda: windows(0, 24, 1, 1), "n_segments"),
    ]
    for i, (call, word) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({word}): returned {rc}"
        with pytest.raises(_lib.LsmHipError, match=word):
            _lib.check(rc, "refused")
    torch.cuda.synchronize()
    assert bool((rec == FILL32).all()) and bool((feats == -7.0).all()), "a refused call wrote to its outputs"
    # the Python layer refuses host counts out of range before it calls the library
    for bad in ((13, 0, 0), (0, -1, 0), (1, 2)):
        with pytest.raises(ValueError):
            net.run_stream_records(r, 8, bad)
    with pytest.raises(ValueError):
        net.segment_features(rec[:, :12], 8, ALL_KEYS, segments=(13, 0, 0))
    # 65535 steps per window is the last accepted; the handle still works
    assert windows(4, 21845, 3, 1) == 0 and windows(4, 21846, 3, 1) == -1
    torch.cuda.synchronize()
    _RAN.add("dense" if "dense" in case.offered else case.offered[0])
    case.net.set_kernel("dense" if "dense" in case.offered else case.offered[0])
    try:
        got = net.segment_features(net.run_stream_records(r, 24)[0], 24, ALL_KEYS).cpu().numpy()
    finally:
        case.net.set_kernel("auto")
    np.testing.assert_array_equal(got, seg._ref_rows(case, 24))


def test_every_family_ran(torch_cuda):
    """Last in the module: over the four shapes every kernel family ran a stream launch."""
    missing = [kernel for kernel in _base().KERNELS if kernel not in _RAN]
    assert not missing, f"kernel families that never ran a stream launch: {missing} (ran: {sorted(_RAN)})"
