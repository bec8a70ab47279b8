"""Stream endpointing on the GPU (SPEC.md 1.17; `lsm_endpoint_stream_f32`, `frontend.EndpointStream`,
`pipeline.UtteranceBank`, `pipeline.utterances_from_recordings`).  Every launch is compared byte for byte with the NumPy
restatement (tests/endpoint_restatement.py) over the seeded pushes of test_endpoint_host.py, whose coverage a CPU test asserts:
every output array, the regions a launch must leave alone (they hold 0xAA before it) and the ones it must write as +0.0 / 0.
Every buffer lies in the middle of 0xAA bytes that must keep their fill, rows hold NaN behind a stream's hops, and the hop
counts go through the ABI as they are, INT32_MIN and INT32_MAX included: the kernel clamps them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import endpoint_restatement as ER  # noqa: E402
import test_endpoint_host as EH  # noqa: E402

pytestmark = pytest.mark.gpu

HOP = 160
FILL = 0xAA
GUARD = 64
NAMES = ("audio", "bins", "first", "flags", "count", "energy", "active")


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


class _Guarded:
    """``nbytes`` of device memory in the middle of FILL bytes, at ``skew`` bytes behind a 256-byte boundary."""

    def __init__(self, torch, nbytes, skew=0, content=None):
        self.n, self.at = nbytes, 256 + skew
        self.buf = torch.full((self.at + nbytes + GUARD + 256,), FILL, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.at += (-base) % 256
        self.ptr = base + self.at
        if content is not None:
            self.put(content)

    def put(self, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        assert len(raw) == self.n
        self.buf[self.at:self.at + self.n] = self.buf.new_tensor(raw)

    def zero(self):
        self.buf[self.at:self.at + self.n] = 0

    def bytes(self):
        got = self.buf.cpu().numpy()
        assert (got[:self.at] == FILL).all() and (got[self.at + self.n:] == FILL).all(), "written outside the buffer"
        return got[self.at:self.at + self.n]


def _push(torch, case, k, state_in, state_out, skew=0, only=NAMES, stream=None):
    """Push ``k`` of a case through the C ABI into buffers prefilled like the restatement's: ``{name: bytes}``."""
    p, U = case["p"], case["max_utts"]
    audio = case["audio"][k]
    n, n_hops = audio.shape[0], audio.shape[1] // HOP
    src = _Guarded(torch, audio.nbytes, skew, audio)
    hops = None if case["hops"][k] is None else torch.tensor(case["hops"][k], dtype=torch.int32, device="cuda")
    fin = None if case["finish"][k] is None else torch.tensor(case["finish"][k], dtype=torch.int32, device="cuda")
    pre = EH.prefill(case, k)
    out = {name: _Guarded(torch, pre[name].nbytes, skew if name == "audio" else 0, pre[name]) for name in NAMES
           if name in only or name in ("audio", "bins")}
    ptr = lambda name: C.c_void_p(out[name].ptr) if name in out else None      # noqa: E731
    rc = _lib_().lsm_endpoint_stream_f32(
        C.c_void_p(src.ptr), n, n_hops, C.c_void_p(hops.data_ptr()) if hops is not None else None,
        C.c_void_p(fin.data_ptr()) if fin is not None else None, C.c_double(p["ratio"]), C.c_double(p["floor"]), p["W"], p["P"],
        p["G"], p["A"], p["M"], C.c_void_p(state_in.ptr) if state_in is not None else None,
        C.c_void_p(state_out.ptr) if state_out is not None else None, U, ptr("audio"), ptr("bins"), ptr("first"), ptr("flags"),
        ptr("count"), ptr("energy"), ptr("active"), stream)
    assert rc == 0, _lib_().lsm_last_error().decode()
    torch.cuda.synchronize()
    src.bytes()                                                     # the input keeps its guards too
    return {name: g.bytes().tobytes() for name, g in out.items()}


def _state(torch, p, n=EH.N_STREAMS, zero=True):
    g = _Guarded(torch, n * int(_lib_().lsm_endpoint_state_bytes(p["W"], p["M"])))
    if zero:
        g.zero()
    return g


@pytest.mark.parametrize("n_hops", EH.GPU_HOPS)
def test_every_push_equals_the_restatement(torch_cuda, n_hops):
    """5 streams, six pushes of 1, 7, 64 and 65 hops (one energy tile, and one bin more), every (W, P, G, M) of the grid.  The
    state goes in place (even combinations) or from block to block (odd ones: the first push reads NULL, and the blocks are
    not zeroed: a launch writes every byte of state_out); odd combinations also put the audio and the slots 4 bytes behind a
    16-byte boundary, so both copy paths run."""
    torch = torch_cuda
    emitted = 0
    for combo in range(len(EH.GPU_COMBOS)):
        case = EH.gpu_case(n_hops, combo)
        want, _ = EH.gpu_expected(n_hops, combo)
        in_place = combo % 2 == 0
        blocks = [_state(torch, case["p"])] if in_place else [_state(torch, case["p"], zero=False) for _ in range(2)]
        for k in range(EH.N_PUSHES):
            if in_place:
                s_in = s_out = blocks[0]
            else:
                s_in, s_out = (None if k == 0 else blocks[(k + 1) % 2]), blocks[k % 2]
            got = _push(torch, case, k, s_in, s_out, skew=0 if in_place else 4)
            for name in NAMES:
                assert got[name] == want[k][name].tobytes(), (combo, EH.GPU_COMBOS[combo], k, name)
            for b in blocks:
                b.bytes()
            emitted += int(want[k]["count"].sum())
        # every stream finished with the last push: its block is all zeros
        assert not blocks[0 if in_place else (EH.N_PUSHES - 1) % 2].bytes().any()
    assert emitted >= (3 if n_hops == 1 else 30)


def test_null_outputs_leave_the_others_and_an_idle_stream_keeps_its_block(torch_cuda):
    torch = torch_cuda
    case = EH.gpu_case(64, 5)
    want, _ = EH.gpu_expected(64, 5)
    assert want[0]["count"].sum() >= 3
    full = _push(torch, case, 0, None, None)
    bare = _push(torch, case, 0, None, None, only=("audio", "bins"))
    assert set(bare) == {"audio", "bins"} and all(bare[n] == full[n] == want[0][n].tobytes() for n in bare)
    # h_b = 0 without finish copies the block byte for byte, whatever it holds; a finished stream's block is zeros
    p = case["p"]
    size = int(_lib_().lsm_endpoint_state_bytes(p["W"], p["M"]))
    junk = np.random.default_rng(3).integers(0, 256, size=(EH.N_STREAMS, size), dtype=np.uint8)
    junk[3] = 0                                                     # the stream that finishes: a fresh one
    s_in, s_out = _state(torch, p), _state(torch, p, zero=False)
    s_in.put(junk)
    idle = dict(case, hops=[[0, -1, EH.I32_MIN, 0, 0]], finish=[[0, 0, 0, 1, 0]], audio=[case["audio"][0]])
    got = _push(torch, idle, 0, s_in, s_out)
    after = s_out.bytes().reshape(EH.N_STREAMS, size)
    for b in (0, 1, 2, 4):
        assert after[b].tobytes() == junk[b].tobytes()
    assert not after[3].any() and s_in.bytes().tobytes() == junk.tobytes()
    assert not np.frombuffer(got["bins"], dtype=np.int32).reshape(EH.N_STREAMS, -1)[[0, 1, 2, 4]].any()


def _collect(utt, n, found):
    """The utterances of one push (`frontend.Utterances`) appended per stream as ``(first, bins, flags, raw samples)``."""
    count = utt.count.cpu().numpy()
    U = utt.bins.shape[0] // n
    bins, first, flags = (t.cpu().numpy().reshape(n, U) for t in (utt.bins, utt.first, utt.flags))
    audio = utt.audio.cpu().numpy().reshape(n, U, -1)
    assert (bins[np.arange(U)[None, :] >= count[:, None]] == 0).all()
    for b in range(n):
        for u in range(int(count[b])):
            found[b].append((int(first[b, u]), int(bins[b, u]), int(flags[b, u]), audio[b, u, :HOP * int(bins[b, u])].tobytes()))
            assert not audio[b, u, HOP * int(bins[b, u]):].any()


def test_streams_cut_anywhere_give_the_uncut_run(torch_cuda):
    """`frontend.EndpointStream`: five streams of 120 bins in one push, in pushes of 7 hops with random counts (0 included)
    and hop by hop -- the same utterances, and the restatement's."""
    from lsm_speech_classifier_amd import frontend
    rng = np.random.default_rng(21)
    n, n_bins = 5, 120
    W, P, G, M = 8, 3, 4, 12
    lines = [EH.timeline(n_bins, G, M, rng, sp) for sp in (None, "nan", "huge", "negzero", None)]
    kw = dict(top_db=20.0, floor_db=-52.0, window_bins=W, pad_bins=P, hang_bins=G, min_span_bins=3, max_bins=M)
    p = ER.params(ER.ratio_of(20.0), ER.floor_of(-52.0), W, P, G, 3, M)
    with np.errstate(all="ignore"):
        want = EH._all_utterances(lines, p, lambda nb, r: [nb], rng)
    assert sum(len(w) for w in want) >= 15

    def run(H, counts_of):
        ep = frontend.EndpointStream(n, **kw)
        assert ep.state_bytes % 16 == 0 and ep.max_utterances(H) == ER.max_utterances_padded(H, P, G, M)
        found, at = [[] for _ in range(n)], np.zeros(n, dtype=np.int64)
        while (at < n_bins).any():
            h = np.minimum(counts_of(H), n_bins - at)
            block = np.full((n, H * HOP), np.nan, dtype=np.float32)
            for b in range(n):
                block[b, :h[b] * HOP] = lines[b][at[b] * HOP:(at[b] + h[b]) * HOP]
            at += h
            _collect(ep.push(block, h, (at == n_bins) & (h > 0)), n, found)
        assert not ep.state.any()                                   # every stream finished
        return found

    assert run(n_bins, lambda H: np.full(n, H)) == want
    assert run(7, lambda H: rng.integers(0, H + 1, size=n)) == want
    assert run(1, lambda H: rng.integers(0, 2, size=n)) == want


def test_the_python_layer(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    for bad in (dict(window_bins=0), dict(window_bins=1025), dict(max_bins=2), dict(pad_bins=100), dict(hang_bins=2),
                dict(hang_bins=1025), dict(min_span_bins=2), dict(min_span_bins=101), dict(top_db=0.0), dict(floor_db=float("nan"))):
        with pytest.raises(ValueError):
            frontend.EndpointStream(2, **bad)
    with pytest.raises(ValueError, match="n_streams"):
        frontend.EndpointStream(0)
    ep = frontend.EndpointStream(2, top_db=None, floor_db=None, window_bins=1, pad_bins=0, hang_bins=1, min_span_bins=3, max_bins=3)
    assert ep.ratio == 0.0 and ep.floor == 0.0 and ep.params["max_bins"] == 3
    for name in ("window_bins", "max_bins"):                        # a state block means what it says only under these two
        with pytest.raises(AttributeError):
            setattr(ep, name, 5)
    for bad in (np.zeros((3, HOP), np.float32), np.zeros((2, HOP + 1), np.float32), np.zeros((2, 0), np.float32),
                np.zeros((2, 4097 * HOP), np.float32)):
        with pytest.raises(ValueError, match="audio must be"):
            ep.push(bad)
    x = np.zeros((2, 4 * HOP), np.float32)
    for bad in ([1, 5], [-1, 0], [1], np.array([1.0, 2.0])):
        with pytest.raises(ValueError, match="hops must be"):
            ep.push(x, bad)
    with pytest.raises(ValueError, match="finish must be"):
        ep.push(x, None, [0, 2])
    with pytest.raises(ValueError, match="int32"):
        ep.push(x, torch.zeros(2, dtype=torch.int64, device="cuda"))
    x[:, :3 * HOP] = 0.5
    a = ep.push(x)                                                  # three active bins: a cut at bin 2
    assert a.count.tolist() == [1, 1] and a.bins.reshape(2, -1)[:, 0].tolist() == [3, 3] and a.flags.reshape(2, -1)[:, 0].tolist() == [1, 1]
    assert ep.push(x) is a                                          # the buffers belong to the bank, one set per H
    assert a.first.reshape(2, -1)[:, 0].tolist() == [4, 4]
    ep.reset([1])
    assert ep.push(x, torch.tensor([4, 4], dtype=torch.int32, device="cuda")).first.reshape(2, -1)[:, 0].tolist() == [8, 0]
    with pytest.raises(ValueError, match="outside"):
        ep.reset([2])


def test_a_captured_push_replays_to_the_same_bytes(torch_cuda):
    """One linear launch, captured once and replayed twice from a zeroed state."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    case = EH.gpu_case(64, 5)
    W, P, G, M = EH.GPU_COMBOS[5]
    ep = frontend.EndpointStream(EH.N_STREAMS, top_db=20.0, floor_db=-52.0, window_bins=W, pad_bins=P, hang_bins=G, max_bins=M)
    x = torch.from_numpy(case["audio"][0]).cuda()
    hops = torch.tensor([64, 64, 30, 64, 0], dtype=torch.int32, device="cuda")
    fin = torch.tensor([0, 1, 0, 0, 0], dtype=torch.int32, device="cuda")
    eager = ep.push(x, hops, fin)                                   # also the first launch: nothing left to set up in capture
    torch.cuda.synchronize()
    want = [t.cpu().numpy().tobytes() for t in eager]
    state = ep.state.cpu().numpy().tobytes()
    assert int(eager.count.sum()) >= 3
    p = ER.params(ER.ratio_of(20.0), ER.floor_of(-52.0), W, P, G, 3, M)
    with np.errstate(all="ignore"):
        ref = ER.push([ER.fresh() for _ in range(5)], case["audio"][0], hops.tolist(), fin.tolist(), p, ep.max_utterances(64))
    assert ER.listing(ref) == ER.listing({k: v.cpu().numpy().reshape(ref[k].shape) for k, v in eager._asdict().items()})
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    ep.state.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = ep.push(x, hops, fin)
    assert captured is eager
    for replay in range(2):
        ep.state.zero_()
        for t in captured:                                          # what a launch leaves alone is what it finds: the eager push
            t.zero_()                                               # found zeros behind the counts
        graph.replay()
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in captured] == want, replay
        assert ep.state.cpu().numpy().tobytes() == state


# ---- audio streams to utterance rows and labels -------------------------------------------------------------------------------
KEYS = ["spike_counts", "spike_variances", "last_spike_times", "mean_isi"]


def _words(n_bins, rng, M):
    """A stream of ``n_bins`` bins: tone bursts of 4 .. M + 3 bins (some longer than M: forced cuts) between stretches of faint
    noise of 5 .. 9 bins."""
    x = (0.0002 * rng.standard_normal(n_bins * HOP)).astype(np.float32)
    at = int(rng.integers(0, 6))
    while at < n_bins:
        hi = min(n_bins, at + int(rng.integers(4, M + 4)))
        t = np.arange((hi - at) * HOP) / 16000.0
        f0, f1 = rng.uniform(200, 3000, size=2)
        x[at * HOP:hi * HOP] += (0.3 * np.sin(2 * np.pi * (f0 + (f1 - f0) * t / max(t[-1], 1e-3)) * t)
                                 * (0.4 + np.abs(np.sin(2 * np.pi * 9 * t))) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)
        at = hi + int(rng.integers(5, 10))
    return x


def _model(n_out, n_classes=4, seed=0, params=None):
    from lsm_speech_classifier_amd import readout
    rng = np.random.default_rng(seed)
    D = len(KEYS) * n_out
    return readout.LinearModel(rng.standard_normal(D), rng.uniform(0.5, 2.0, D), rng.standard_normal((n_classes, D)),
                               rng.standard_normal(n_classes), np.arange(n_classes), KEYS, n_out, params=params)


def _bank_case(torch, fe, net, fused, monkeypatch):
    """Three pushes of 40 hops on 5 streams through `UtteranceBank.push_scores`, with ``compact`` off and on: every emitted
    utterance's row and logits equal, bit for bit, `features_from_utterances` + `score_rows` on its slice taken alone; with
    ``compact`` off nothing is read on the host between the push and the scores."""
    from lsm_speech_classifier_amd import frontend, pipeline, readout
    n, H, M = 5, 40, fe.time_bins
    rng = np.random.default_rng(77)
    lines = [_words(3 * H, rng, M) for _ in range(n)]
    kw = dict(top_db=20.0, floor_db=-50.0, window_bins=8, pad_bins=1, hang_bins=3, min_span_bins=3, max_bins=M)
    ro = readout.DeviceReadout(_model(net.num_output_neurons), net.device)
    calls = []
    real = pipeline.step_fused_ragged
    monkeypatch.setattr(pipeline, "step_fused_ragged", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    seen = {}
    for compact in (False, True):
        bank = pipeline.UtteranceBank(frontend.EndpointStream(n, **kw), fe, net, KEYS, readout=ro, fused=fused)
        rows_of, found = [], []
        for k in range(3):
            block = np.stack([x[k * H * HOP:(k + 1) * H * HOP] for x in lines])
            x = torch.from_numpy(block).cuda()
            fin = torch.tensor([1 if k == 2 else 0] * n, dtype=torch.int32, device="cuda")
            if not compact:
                with monkeypatch.context() as mp:
                    def boom(*a, **k_):
                        raise AssertionError("a device value was read on the host between the push and the scores")
                    for method in ("cpu", "item", "numpy", "tolist", "__bool__", "__int__", "__float__"):
                        mp.setattr(torch.Tensor, method, boom)
                    out = bank.push_scores(x, None, fin)
                    rows = bank._rows(bank.endpoint._outputs[H], False)
            else:
                out = bank.push_scores(x, None, fin, compact=True)
                rows = bank._rows(bank.endpoint._outputs[H], True)
            logits, labels, bins, first, flags = (t.cpu().numpy() for t in out)
            audio = bank.endpoint._outputs[H].audio.cpu().numpy()
            rows = rows.cpu().numpy()
            for slot in np.nonzero(bins)[0]:
                found.append((slot, int(first[slot]), int(bins[slot]), int(flags[slot]), audio[slot, :HOP * int(bins[slot])].copy()))
                rows_of.append((rows[slot], logits[slot], int(labels[slot])))
        assert len(found) >= 8 and any(f[3] & 1 for f in found) and any(f[3] & 2 for f in found)
        want = pipeline.features_from_utterances([f[4] for f in found], fe, net, KEYS)
        want_logits, want_labels = ro.score_rows(want)
        want, want_logits, want_labels = want.cpu().numpy(), want_logits.cpu().numpy(), want_labels.cpu().numpy()
        live = want[want.any(axis=1)]
        assert len(live) >= 5 and len({w.tobytes() for w in live}) == len(live)      # the reference tells the utterances apart
        for i, (row, lg, lab) in enumerate(rows_of):
            assert row.view(np.uint32).tobytes() == want[i].view(np.uint32).tobytes(), (compact, i)
            assert lg.view(np.uint64).tobytes() == want_logits[i].view(np.uint64).tobytes() and lab == int(want_labels[i])
        seen[compact] = [(f[0], f[1], f[2], f[3], f[4].tobytes()) for f in found]
    assert seen[False] == seen[True]
    return len(calls)


def _small_net(c):
    """The small reservoir of the ragged feature tests at half the membrane threshold, so that clips of a dozen bins drive it."""
    from lsm_speech_classifier_amd import reservoir as R, snn
    n, k, n_out = 64, 16, 32
    return snn.SNN(None, reservoir=R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                                        mean_weight=2.0 / (k // 2), refractory_period=2,
                                                                        membrane_threshold=1.0), c))


def test_utterance_bank_on_the_split_route(torch_cuda, monkeypatch):
    """16 filters, N = 64, max_bins = 12: `encode_ragged` + `run_batch(lengths=...)` on the slot batch."""
    from lsm_speech_classifier_amd import frontend, pipeline
    fe = frontend.SpikeFrontEnd(16, "gammatone", redundancy=2, thresholds=[0.40, 0.55, 0.70, 0.85], gap=0.1, time_bins=12,
                                n_samples=HOP * 12)
    net = _small_net(fe.n_channels)
    assert _bank_case(torch_cuda, fe, net, None, monkeypatch) == 0
    with pytest.raises(ValueError, match="fused=True"):
        pipeline.UtteranceBank(frontend.EndpointStream(5, max_bins=12, pad_bins=1, hang_bins=3), fe, net, KEYS, fused=True).push(
            np.zeros((5, HOP), np.float32))
    # a front end of another shape is refused with the reason
    with pytest.raises(ValueError, match="max_bins = 20"):
        pipeline.UtteranceBank(frontend.EndpointStream(5, max_bins=20), fe, net, KEYS)
    other = frontend.SpikeFrontEnd(16, "gammatone", redundancy=2, time_bins=12, n_samples=2000)
    with pytest.raises(ValueError, match="n_samples"):
        pipeline.UtteranceBank(frontend.EndpointStream(5, max_bins=12), other, net, KEYS)
    with pytest.raises(ValueError, match="readout"):
        pipeline.UtteranceBank(frontend.EndpointStream(5, max_bins=12), fe, net, KEYS).push_scores(np.zeros((5, HOP), np.float32))


def test_utterance_bank_on_the_fused_route(torch_cuda, oracle_c, monkeypatch):
    """128 filters, 16 bins, the reservoir of the one-launch step's tests: there the ragged form is served and the slot batch
    is one launch per push (and one more per compact push)."""
    import step_fused_forms_ref as REF
    from lsm_speech_classifier_amd import frontend, pipeline, snn
    fe = frontend.SpikeFrontEnd(128, "gammatone", thresholds=REF.thresholds(4), time_bins=16, n_samples=2560)
    net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, 128, 16, 4, 160, 384))
    assert pipeline.step_fused_supported(fe, net, 5 * frontend.endpoint_max_utterances(40, 1, 3, 16), "ragged")
    assert _bank_case(torch_cuda, fe, net, None, monkeypatch) >= 6


def test_utterances_from_recordings_equal_the_restatement(torch_cuda):
    from lsm_speech_classifier_amd import pipeline
    rng = np.random.default_rng(9)
    recs = [_words(150, rng, 12), _words(95, rng, 12)[:95 * HOP - 57], _words(230, rng, 12)]
    kw = dict(top_db=20.0, floor_db=-50.0, window_bins=8, pad_bins=1, hang_bins=3, min_span_bins=3, max_bins=12)
    p = ER.params(ER.ratio_of(20.0), ER.floor_of(-50.0), 8, 1, 3, 3, 12)
    utts, table = pipeline.utterances_from_recordings(recs, kw, chunk_hops=64)
    at = 0
    for r, rec in enumerate(recs):
        with np.errstate(all="ignore"):
            want = ER.cut_recording(rec, p, chunk_hops=64)
        assert len(want) >= 5
        for first, bins, flags, samples in want:
            assert table[at].tolist() == [r, first, bins, flags] and utts[at].tobytes() == samples.tobytes(), (r, at)
            at += 1
    assert at == len(utts) == len(table) and any(table[:, 3] & 1) and any(table[:, 3] & 2)


def test_classify_prints_one_line_per_utterance(torch_cuda, tmp_path, capsys):
    """`classify.py --stream --endpoint` on a wav file of 150 bins: the lines' times are the restatement's utterances (pushes
    of 500 ms, the default window of 100 bins), the labels those of the clip route on the restatement's slices."""
    import classify
    from scipy.io import wavfile
    from lsm_speech_classifier_amd import frontend, pipeline, readout, reservoir as R
    fe = frontend.SpikeFrontEnd(16, "gammatone", redundancy=2, thresholds=[0.40, 0.55, 0.70, 0.85], gap=0.1, time_bins=12,
                                n_samples=HOP * 12)
    sim = R.SimulationParams(num_neurons=64, num_output_neurons=32, small_world_graph_k=16, mean_weight=0.25, refractory_period=2,
                             membrane_threshold=1.0)
    model = _model(32, params=pipeline.model_params(fe, sim))
    x = _words(150, np.random.default_rng(4), 12)
    path = str(tmp_path / "stream.wav")
    wavfile.write(path, 16000, x)                                   # float32 PCM: decoded to the same samples
    a = classify.build_parser().parse_args(["--model", "m.npz", "--stream", "--endpoint", "--endpoint-top-db", "20",
                                            "--endpoint-floor-db", "-50", "--endpoint-pad-ms", "10", "--endpoint-hang-ms", "30", path])
    lines = classify.classify_utterances(model, [path], classify.endpoint_from_args(a, 12))
    with np.errstate(all="ignore"):
        want = ER.cut_recording(x, ER.params(ER.ratio_of(20.0), ER.floor_of(-50.0), 100, 1, 3, 3, 12), chunk_hops=50)
    assert len(want) >= 5 and [(t0, t1) for _, t0, t1, _ in lines] == [(10.0 * f, 10.0 * (f + b)) for f, b, _, _ in want]
    fe2, net = pipeline.pipeline_from_params(model.params)
    rows = pipeline.features_from_utterances([w[3] for w in want], fe2, net, KEYS)
    labels = readout.DeviceReadout(model, net.device).score_rows(rows)[1].cpu().numpy()
    assert [cls for _, _, _, cls in lines] == [classify.class_name(model, int(v)) for v in labels]
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == len(want) and all(ln.startswith(path + "\t") and ln.count("\t") == 3 for ln in printed)
