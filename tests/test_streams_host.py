"""Open-ended streams (SPEC.md 4d): what can be checked without a GPU -- the new public header and its ctypes table, the
build identity, `pipeline.stream_window_plan` against a brute-force enumeration of windows, the argument checks of
`SNN.run_stream_records`, `pipeline.CarryBuffer` against a list per stream, and a NumPy restatement of "ragged records -> merge fold -> feature_value" against the oracle's
`feature_row` on slices of one oracle spike matrix."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_EXPORTS = {"lsm_reservoir_run_stream": 16, "lsm_segment_features_ragged": 12}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def test_the_new_header_declares_the_two_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_streams.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.STREAM_SYMBOLS == tuple(_lib.STREAM_SIGS) and set(_lib.STREAM_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        proto = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.STREAM_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is _lib.c_int
        # every pointer parameter is a void pointer in the table, every scalar an int (the workspace size a long)
        for p, ctype in zip(params, args):
            want = _lib.c_void if "*" in p else (_lib.C.c_long if p.startswith("long ") else _lib.c_int)
            assert ctype is want, f"{name}: {p}"
    proto = re.search(r"int lsm_reservoir_run_stream\((.*?)\);", header, re.S).group(1)
    assert "first_step" not in proto and "key_ids" not in proto and "const int32_t *clip_segments" in proto


def test_the_first_header_and_its_table_stay_as_they_are():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    declared = set(re.findall(_DECLARED, header, re.M)) | set(re.findall(r"^const char \*(lsm_[a-z0-9_]+)\s*\(", header, re.M))
    assert len(_lib.EXPORTED_SYMBOLS) == 38
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert not set(NEW_EXPORTS) & set(_lib.EXPORTED_SYMBOLS) and not set(NEW_EXPORTS) & set(_lib._SIGS)


def test_the_library_exports_both_symbols():
    from lsm_speech_classifier_amd import build
    path = build.lib_path()
    assert os.path.exists(path), f"{path} is not built"
    blob = open(path, "rb").read()
    for name in NEW_EXPORTS:
        assert name.encode() + b"\0" in blob, f"{name} is not in the library's symbol table"
    try:
        lib = ctypes.CDLL(path)
    except OSError:
        return                                  # no HIP runtime to resolve against here: the symbol table was read above
    for name in NEW_EXPORTS:
        assert getattr(lib, name) is not None


def test_the_build_identity_covers_the_new_header(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_streams.h" in build.PUBLIC_HEADERS and "lsm_hip.h" in build.PUBLIC_HEADERS
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    path = inc / "lsm_hip_streams.h"
    data = bytearray(path.read_bytes())
    data[len(data) // 2] ^= 1
    path.write_bytes(bytes(data))
    assert build.source_id(str(inc)) != build.source_id()


# ---- stream_window_plan against the enumeration of windows ---------------------------------------------------------------
def _enumerate(seen, new, K, H):
    """Windows [w * H, w * H + K) completed by the segments seen + 1 .. seen + new, one by one, and the records from the
    start of the first window still open."""
    total = seen + new
    done, w = 0, 0
    while w * H + K <= total:
        done += 1 if w * H + K > seen else 0
        w += 1
    return done, sum(1 for g in range(total) if g >= w * H)


def test_stream_window_plan_equals_the_enumeration():
    from lsm_speech_classifier_amd import pipeline
    rng = np.random.RandomState(11)
    for K in range(1, 6):
        for H in range(1, K + 1):
            for trial in range(4):
                seen, emitted = 0, 0
                for new in [0] + rng.randint(0, 2 * K + 3, size=40).tolist() + [0, 0, 1]:
                    n_windows, keep = pipeline.stream_window_plan(seen, new, K, H)
                    assert (n_windows, keep) == _enumerate(seen, new, K, H), (K, H, seen, new)
                    assert 0 <= keep <= K - 1
                    seen += new
                    emitted += n_windows
                assert emitted == ((seen - K) // H + 1 if seen >= K else 0)
            # arrays, element by element
            seen_a, new_a = rng.randint(0, 50, size=16), rng.randint(0, 9, size=16)
            nw, keep = pipeline.stream_window_plan(seen_a, new_a, K, H)
            assert [(int(a), int(b)) for a, b in zip(nw, keep)] == [_enumerate(int(s), int(n), K, H)
                                                                   for s, n in zip(seen_a, new_a)]
    for K, H in ((1, 2), (3, 4), (0, 1), (2, 0)):
        with pytest.raises(ValueError):
            pipeline.stream_window_plan(0, 1, K, H)
    with pytest.raises(ValueError):
        pipeline.stream_window_plan(-1, 1, 2, 1)


# ---- the argument checks of run_stream_records: before any library call --------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _net_without_a_gpu():
    import torch
    from lsm_speech_classifier_amd import snn
    net = snn.SNN.__new__(snn.SNN)                  # no handle, no device: every check below happens on the host
    net.lib = _NoLibrary()
    net._handle = None
    net.device = torch.device("cpu")
    net.n_channels, net.num_neurons, net.num_output_neurons = 4, 64, 8
    return net


def test_run_stream_records_checks_its_arguments_on_the_host():
    import torch
    net = _net_without_a_gpu()
    spikes = np.zeros((3, 4, 24), dtype=np.uint8)
    for segments in ((4, 0, 0), (0, -1, 0), (1, 2), (1, 2, 3, 0), (1.0, 2.0, 3.0), torch.tensor([1, 2, 3]),
                     torch.tensor([1, 2], dtype=torch.int32), np.array([[1, 2, 3]])):
        with pytest.raises(ValueError, match="segments"):
            net.run_stream_records(spikes, 8, segments)
    for S in (0, -8, 5, 48):
        with pytest.raises(ValueError, match="segment_steps"):
            net.run_stream_records(spikes, S, (0, 0, 0))
    with pytest.raises(ValueError, match="spikes"):
        net.run_stream_records(np.zeros((3, 5, 24), dtype=np.uint8), 8)
    # in range: the static check hands back the counts (a device tensor would not be read)
    assert net._host_segments((3, 0, 1), 3, 3).tolist() == [3, 0, 1]
    assert net._host_segments(torch.tensor([3, 0, 1], dtype=torch.int32), 3, 3).tolist() == [3, 0, 1]
    # segment_features(segments=): the same check, before the library
    records = torch.zeros((3, 3, 8, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="segments"):
        net.segment_features(records, 8, segments=(4, 0, 0))


def test_launch_methods_keep_their_own_refusals_on_the_host():
    """What the launch methods' shared argument steps must not blur: the noun in a count's refusal, which exception a bad
    ``segment_steps`` raises from which method, and the ``state_out`` / ``stats_out`` refusals of all three launch
    methods -- each before the library is called (``_NoLibrary`` fails the test otherwise)."""
    import torch
    from lsm_speech_classifier_amd import _lib
    net = _net_without_a_gpu()
    spikes = np.zeros((3, 4, 24), dtype=np.uint8)
    for lengths in ((25, 0, 0), (0, -1, 0), (1, 2), (1, 2, 3, 0), (1.0, 2.0, 3.0), torch.tensor([1, 2, 3]),
                    torch.tensor([1, 2], dtype=torch.int32)):
        with pytest.raises(ValueError, match="lengths"):
            net.run_batch(spikes, lengths=lengths, longest_first=False)
    for S in (0, 5, 48):
        with pytest.raises(_lib.LsmHipError, match="segment_steps"):
            net.run_segment_records(spikes, S)
        with pytest.raises(_lib.LsmHipError, match="segment_steps"):
            net.run_segments(spikes, S)
        with pytest.raises(ValueError, match="segment_steps"):
            net.run_stream_records(spikes, S)
    launches = (lambda **kw: net.run_batch(spikes, longest_first=False, **kw),
                lambda **kw: net.run_segment_records(spikes, 8, **kw),
                lambda **kw: net.run_stream_records(spikes, 8, **kw))
    for launch in launches:
        with pytest.raises(ValueError, match="state_out needs state"):
            launch(state_out=object())
        with pytest.raises(ValueError, match="stats_out must be"):
            launch(stats_out=torch.zeros((3, 3), dtype=torch.int32))


# ---- NumPy restatement: ragged records, merge fold, feature_value ----------------------------------------------------------
def test_ragged_records_fold_to_the_oracles_rows_on_slices(oracle_c):
    """Per-clip counts: clip b's G_b records are the records of its first G_b * S steps (what it ran), window w < W_b folds
    records wH .. wH + K - 1, and the rows equal the oracle's rows on slices; nothing at g >= G_b or w >= W_b is made."""
    import test_segments_host as host                       # _segment_records, _window_row
    from oracle import ref_numpy
    from lsm_speech_classifier_amd import reservoir as R
    n, k, n_out, c, T = 256, 50, 100, 40, 96
    res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                               mean_weight=2.0 / (k // 2), refractory_period=2), c)
    burst = int(res.burst_isi_max)
    sms = [oracle_c.lif_run(res, (np.random.RandomState(b).random_sample((c, T)) < 0.35).astype(np.uint8), host.ALL_KEYS)[1]
           for b in range(3)]
    for S, counts, K, H in ((8, (12, 5, 0), 3, 2), (8, (1, 12, 7), 1, 1), (24, (4, 1, 0), 2, 1), (1, (96, 37, 0), 5, 4)):
        G = T // S
        for b, (sm, g_b) in enumerate(zip(sms, counts)):
            g_b = min(max(g_b, 0), G)
            ran = sm[:g_b * S]                              # input behind L_b influences nothing: the clip alone, L_b steps
            rec = host._segment_records(ran[:, res.out_idx], S, burst)
            assert rec.shape[0] == g_b
            np.testing.assert_array_equal(rec, host._segment_records(sm[:, res.out_idx], S, burst)[:g_b])
            w_b = (g_b - K) // H + 1 if g_b >= K else 0
            assert w_b <= (G - K) // H + 1
            for keys in (host.ALL_KEYS, ['burst_counts', 'spike_variances']):
                for w in range(w_b):
                    want = ref_numpy.feature_row(sm[w * H * S:(w * H + K) * S], res.out_idx, burst, keys)
                    np.testing.assert_array_equal(host._window_row(rec, w * H, K, S, burst, keys), want,
                                                  err_msg=f"S={S} clip {b} window {w}")
            assert w_b == 0 or (w_b - 1) * H + K <= g_b < w_b * H + K      # the last window fits, one more would not


# ---- StreamBank's bookkeeping with a stand-in reservoir: which records reach which window --------------------------------
class _LabelNet:
    """Stands in for SNN on the CPU: a segment's "record" is the label the test wrote into the first step of that segment
    of the raster (channel 0 + 256 * channel 1), and a window's "row" is the labels of the records it folds."""
    num_output_neurons = 1
    num_neurons = 1

    def __init__(self, max_steps):
        import torch
        from lsm_speech_classifier_amd import snn
        self.device = torch.device("cpu")
        self._host_segments = snn.SNN._host_segments
        self.max = max_steps
        self.launches = []

    def new_state(self, n):
        import torch
        from lsm_speech_classifier_amd import snn
        return snn.ReservoirState(torch.zeros((n, 64), dtype=torch.uint8), 1, 1)

    def _max_steps_cached(self, n_clips, waves_per_clip=0):
        return self.max

    def run_stream_records(self, spikes, S, segments=None, state=None, **kw):
        import torch
        B, _, T = spikes.shape
        assert T <= self.max and T % S == 0
        rec = torch.zeros((B, T // S, 1, 4), dtype=torch.int32)
        self.launches.append(np.asarray(segments).tolist())
        for b in range(B):
            for g in range(int(segments[b])):
                rec[b, g, 0, 0] = int(spikes[b, 0, g * S]) + 256 * int(spikes[b, 1, g * S])
                state.data[b, 0] = 1                                    # the stream has run
        return rec, None, None

    def segment_features(self, records, S, keys, K, H, segments=None):
        import torch
        B, G = records.shape[:2]
        W = (G - K) // H + 1
        rows = torch.zeros((B, W, K), dtype=torch.float32)
        for b in range(B):
            for w in range((int(segments[b]) - K) // H + 1 if segments[b] >= K else 0):
                rows[b, w] = records[b, w * H:w * H + K, 0, 0].float()
        return rows


@pytest.mark.parametrize("K,H", [(1, 1), (3, 2), (3, 3), (4, 1), (5, 2)])
def test_stream_bank_hands_every_window_its_own_records(K, H, monkeypatch):
    import contextlib
    import torch
    from lsm_speech_classifier_amd import pipeline
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())      # the stand-in lives on the CPU
    S, n_streams = 4, 3
    net = _LabelNet(max_steps=5 * S + 3)                                # pushes of more than 5 segments are cut
    bank = pipeline.StreamBank(net, n_streams, S, K, H, ['spike_counts'])
    rng = np.random.RandomState(100 * K + H)
    seen = np.zeros(n_streams, dtype=np.int64)
    got = [[] for _ in range(n_streams)]
    for push in range(30):
        new = rng.randint(0, 9, size=n_streams) * (rng.random_sample(n_streams) < 0.7)
        g_max = int(max(new.max(), rng.randint(0, 3)))
        rasters = np.full((n_streams, 2, g_max * S), 255, dtype=np.uint8)      # what lies behind a stream's steps is never read
        for b in range(n_streams):
            for g in range(new[b]):
                label = seen[b] + g + 1
                rasters[b, 0, g * S], rasters[b, 1, g * S] = label % 256, label // 256
        rows, counts = bank.push(rasters, new)
        want = [pipeline.stream_window_plan(int(seen[b]), int(new[b]), K, H) for b in range(n_streams)]
        assert counts.tolist() == [w[0] for w in want] and bank.tail_count.tolist() == [w[1] for w in want]
        for b in range(n_streams):
            got[b] += rows[b, :counts[b]].tolist()
            assert not rows[b, counts[b]:].any()
        seen += new
        assert bank.seen.tolist() == seen.tolist()
        if push == 14:                                                  # stream 1 ends, a new one takes its slot
            assert got[1] == [[float(w * H + j + 1) for j in range(K)] for w in range(len(got[1]))]
            bank.reset([1])
            seen[1], got[1] = 0, []
            assert not bank.state.data[1].any() and bank.tail_count[1] == 0
    assert all(max(l) * S <= net.max for l in net.launches if l) and len(net.launches) > 30      # long pushes were cut
    for b in range(n_streams):
        n_w = (seen[b] - K) // H + 1 if seen[b] >= K else 0
        assert got[b] == [[float(w * H + j + 1) for j in range(K)] for w in range(n_w)], f"stream {b}"


# ---- CarryBuffer alone: join and keep against a plain list per stream ------------------------------------------------------
@pytest.mark.parametrize("item,dtype", [((2,), "int32"), ((5,), "uint8")])
@pytest.mark.parametrize("G", [0, 1, 4])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_carry_buffer_joins_and_keeps_like_a_list_per_stream(cap, G, item, dtype):
    """12 consecutive pushes on CPU tensors: after every push the joined run is the model's list (kept items, then the new
    ones), the kept buffer is the list's tail, left-aligned, and everything past ``keep[b]`` is zero; one slot is reset in
    the middle."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    n_streams, tdtype = 3, getattr(torch, dtype)
    rng = np.random.RandomState(1000 * cap + 10 * G + len(item))
    carry = pipeline.CarryBuffer(n_streams, cap, item, tdtype, torch.device("cpu"))
    assert carry.kept.shape == (n_streams, cap, *item) and carry.kept.dtype == tdtype and not carry.count.any()
    model = [[] for _ in range(n_streams)]
    for push in range(12):
        counts = rng.randint(0, G + 1, size=n_streams).astype(np.int64)
        new = rng.randint(1, 200, size=(n_streams, G, *item)).astype(dtype)      # non-zero, also behind a stream's count
        run, have = carry.join(torch.from_numpy(new), counts)
        assert run.shape == (n_streams, cap + G, *item) and run.dtype == tdtype and run.is_contiguous()
        for b in range(n_streams):
            model[b] += [new[b, g].tolist() for g in range(counts[b])]
            assert have[b] == len(model[b])
            assert run[b, :have[b]].tolist() == model[b], (push, b)
        keep = np.array([rng.randint(0, min(cap, len(m)) + 1) for m in model], dtype=np.int64)
        carry.keep(run, have, keep)
        assert carry.kept.shape == (n_streams, cap, *item) and carry.kept.dtype == tdtype and carry.kept.is_contiguous()
        assert carry.count.tolist() == keep.tolist() and carry.count is not keep
        for b in range(n_streams):
            model[b] = model[b][len(model[b]) - keep[b]:]
            assert carry.kept[b, :keep[b]].tolist() == model[b], (push, b)
            assert not carry.kept[b, keep[b]:].any(), (push, b)
        if push == 5:                                                   # stream 1 ends, a new one takes its slot
            carry.reset(np.array([1], dtype=np.int64))
            model[1] = []
            assert carry.count[1] == 0 and not carry.kept[1].any()
            assert carry.count[0] == keep[0] and carry.kept[0, :keep[0]].tolist() == model[0]
