"""Readout scores on the device (SPEC.md 6, include/lsm_hip_readout.h): `lsm_readout_rows_f32` against the NumPy restatement
(tests/readout_restatement.py) byte for byte, `lsm_readout_windows` against `lsm_readout_rows_f32` over
`segment_features(..., segments=...)`'s rows byte for byte, `push_scores` of the stream banks against `score_rows(push(...))`
of a twin bank and against the uncut run, and one launch of each under graph capture and replay."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_restatement as RR  # noqa: E402
from test_readout_host import KEYS8, make_case  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS5 = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _readout(n_keys, n_out, n_classes, seed, keys=None):
    from lsm_speech_classifier_amd import readout
    _, mean, scale, coef, intercept = make_case(1, n_keys, n_out, n_classes, seed)
    model = readout.LinearModel(mean, scale, coef, intercept, np.arange(n_classes) + 100, keys or KEYS8[:n_keys], n_out)
    return model, readout.DeviceReadout(model, "cuda")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- lsm_readout_rows_f32 against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [1, 63, 65, 130, 577])
def test_rows_equal_the_restatement_byte_for_byte(torch_cuda, n_out):
    """Lane tails (63, 65), more than one pass over the lanes (65, 130), a single neuron, and 577 = a second chunk of the
    kernel's 512 neurons that ends in a lane tail; every class tile of the launch (1 and 2 classes in one wave, 7 in two waves
    of 4 with the last one partly filled, 12 in three, 64 in eight waves of 8); one row, a few and a few hundred."""
    torch = torch_cuda
    for n_keys in (1, 5, 8):
        for n_classes in (1, 2, 7, 12, 64):
            model, ro = _readout(n_keys, n_out, n_classes, seed=n_out + n_keys + n_classes)
            for n_rows in (1, 3, 257):
                x = make_case(n_rows, n_keys, n_out, n_classes, seed=n_rows)[0]
                assert x.size < 100 or (x == 0).mean() > 0.2            # exact zeros, as after nan_to_num
                bad = n_rows // 2
                x[bad, (n_keys * n_out) // 2] = np.nan
                logits, labels = ro.score_rows(torch.from_numpy(x).cuda())
                want_logits, want_labels = RR.scores(x, model.mean, model.scale, model.coef, model.intercept, n_keys, n_out)
                what = f"n_out={n_out} n_keys={n_keys} C={n_classes} rows={n_rows}"
                assert logits.dtype == torch.float64 and labels.dtype == torch.int32
                assert logits.cpu().numpy().tobytes() == want_logits.tobytes(), what
                assert labels.cpu().numpy().tobytes() == want_labels.tobytes(), what
                assert want_labels[bad] == -1 and (np.delete(want_labels, bad) >= 0).all()


def test_rows_null_outputs_leading_dims_and_classes(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    model, ro = _readout(5, 70, 35, seed=3)                             # 35 classes: five waves of 8, the last with three
    x = make_case(6, 5, 70, 35, seed=8)[0]
    xd = torch.from_numpy(x).cuda()
    logits, labels = ro.score_rows(xd.reshape(2, 3, 350))
    assert tuple(logits.shape) == (2, 3, 35) and tuple(labels.shape) == (2, 3)
    want_logits, want_labels = RR.scores(x, model.mean, model.scale, model.coef, model.intercept, 5, 70)
    assert logits.cpu().numpy().tobytes() == want_logits.tobytes() and labels.cpu().numpy().tobytes() == want_labels.tobytes()
    assert ro.class_of(labels).cpu().numpy().tolist() == (want_labels.reshape(2, 3) + 100).tolist()
    assert ro.class_of(np.array([-1, 0, 34])).tolist() == [-1, 100, 134]
    stream = torch.cuda.current_stream().cuda_stream
    only_logits = torch.full((6, 35), 7.5, dtype=torch.float64, device="cuda")
    only_labels = torch.full((6,), -77, dtype=torch.int32, device="cuda")
    model_args = ro._model_args()
    _lib.check(lib.lsm_readout_rows_f32(*model_args, _ptr(xd), 6, 5, 70, 35, _ptr(only_logits), None, stream))
    _lib.check(lib.lsm_readout_rows_f32(*model_args, _ptr(xd), 6, 5, 70, 35, None, _ptr(only_labels), stream))
    torch.cuda.synchronize()
    assert only_logits.cpu().numpy().tobytes() == want_logits.tobytes()
    assert only_labels.cpu().numpy().tobytes() == want_labels.tobytes()
    with pytest.raises(ValueError, match="features must be float32"):
        ro.score_rows(xd[:, :-1])


# ---- lsm_readout_windows against lsm_readout_rows_f32 ---------------------------------------------------------------------
_SHARED = {}


def _records(torch):
    """A small reservoir and the records of 3 clips of 6 segments of 8 steps, made once."""
    if "records" not in _SHARED:
        from lsm_speech_classifier_amd import reservoir as R, snn, synth
        F = 24
        res = R.build_reservoir(R.SimulationParams(num_neurons=200, num_output_neurons=70, small_world_graph_k=40,
                                                   mean_weight=0.3, refractory_period=2), F)
        net = snn.SNN(None, reservoir=res)
        raster = synth.bernoulli_raster(3, F, 48, 0.25, seed=11)
        records, _, _ = net.run_stream_records(raster, 8)
        torch.cuda.synchronize()
        counts = records[..., 0].cpu().numpy() & 0xFFFF
        assert records.shape == (3, 6, 70, 4) and (counts >= 2).mean() > 0.2, "the output neurons hardly fire"
        _SHARED["records"] = (net, records)
    return _SHARED["records"]


@pytest.mark.parametrize("K,H", [(1, 1), (3, 1), (3, 2), (6, 1)])
@pytest.mark.parametrize("keys,n_classes", [(KEYS5, 12), (KEYS8, 35)], ids=["5keys-12", "8keys-35"])
def test_windows_equal_rows_over_segment_features(torch_cuda, K, H, keys, n_classes):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    net, records = _records(torch)
    model, ro = _readout(len(keys), 70, n_classes, seed=K * 10 + H, keys=keys)
    W = (6 - K) // H + 1
    stream = torch.cuda.current_stream().cuda_stream
    key_ids = np.array([KEYS8.index(k) for k in keys], dtype=np.int32)
    for segments in ([6, 2, 0], None, torch.tensor([-3, 99, 3], dtype=torch.int32, device="cuda")):
        clamped = [6, 6, 6] if segments is None else np.clip(np.asarray(segments.cpu() if torch.is_tensor(segments)
                                                                        else segments), 0, 6).tolist()
        w_b = [(g - K) // H + 1 if g >= K else 0 for g in clamped]
        rows = net.segment_features(records, 8, keys, K, H, segments=np.array(clamped))
        want_logits, want_labels = ro.score_rows(rows)
        # through the Python layer: zeros and -1 behind a clip's windows
        logits, labels = ro.score_windows(net, records, 8, K, H, segments=segments)
        assert tuple(logits.shape) == (3, W, n_classes) and tuple(labels.shape) == (3, W)
        # the raw launch over sentinels: rows at w >= W_b and a clip without segments are left as they are
        raw_logits = torch.full((3, W, n_classes), 7.5, dtype=torch.float64, device="cuda")
        raw_labels = torch.full((3, W), -77, dtype=torch.int32, device="cuda")
        counts = None if segments is None else (segments if torch.is_tensor(segments)
                                                else torch.tensor(segments, dtype=torch.int32, device="cuda"))
        _lib.check(lib.lsm_readout_windows(net._handle, *ro._model_args(), _ptr(records), 3, 6, _ptr(counts), 8, K, H,
                                           C.c_void_p(key_ids.ctypes.data), len(keys), n_classes, _ptr(raw_logits),
                                           _ptr(raw_labels), stream))
        torch.cuda.synchronize()
        for b in range(3):
            n = w_b[b]
            what = f"clip {b}, segments {segments}, K={K} H={H}"
            assert logits[b, :n].cpu().numpy().tobytes() == want_logits[b, :n].cpu().numpy().tobytes(), what
            assert labels[b, :n].cpu().numpy().tobytes() == want_labels[b, :n].cpu().numpy().tobytes(), what
            assert raw_logits[b, :n].cpu().numpy().tobytes() == want_logits[b, :n].cpu().numpy().tobytes(), what
            assert raw_labels[b, :n].cpu().numpy().tobytes() == want_labels[b, :n].cpu().numpy().tobytes(), what
            assert (raw_logits[b, n:] == 7.5).all() and (raw_labels[b, n:] == -77).all(), what
            assert not logits[b, n:].any() and (labels[b, n:] == -1).all(), what
        assert sum(w_b) > 0 and (want_labels[1, :w_b[1]] >= 0).all()
    # the rows differ from window to window: the comparison is not one of constants
    # (the reservoir starts silent: the rows of the first segments may be equal)
    assert w_b[1] == W and len({want_logits[1, w].cpu().numpy().tobytes() for w in range(W)}) >= min(W, 2)


def test_windows_over_more_output_neurons_than_one_chunk(torch_cuda):
    """600 output neurons: the window launch's second chunk (the kernel scales 512 neurons at a time)."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import reservoir as R, snn, synth
    res = R.build_reservoir(R.SimulationParams(num_neurons=640, num_output_neurons=600, small_world_graph_k=40,
                                               mean_weight=0.3, refractory_period=2), 24)
    net = snn.SNN(None, reservoir=res)
    records, _, _ = net.run_stream_records(synth.bernoulli_raster(2, 24, 48, 0.25, seed=12), 8)
    assert ((records[..., 0] & 0xFFFF) >= 2).float().mean() > 0.1
    model, ro = _readout(5, 600, 12, seed=51, keys=KEYS5)
    segments = torch.tensor([6, 4], dtype=torch.int32, device="cuda")
    want_logits, want_labels = ro.score_rows(net.segment_features(records, 8, KEYS5, 3, 1, segments=segments))
    logits, labels = ro.score_windows(net, records, 8, 3, 1, segments=segments)
    for b, n in enumerate((4, 2)):
        assert logits[b, :n].cpu().numpy().tobytes() == want_logits[b, :n].cpu().numpy().tobytes()
        assert labels[b, :n].cpu().numpy().tobytes() == want_labels[b, :n].cpu().numpy().tobytes()
        assert not logits[b, n:].any() and (labels[b, n:] == -1).all()
    assert (want_labels[0] >= 0).all() and len({want_logits[0, w].cpu().numpy().tobytes() for w in range(4)}) >= 2


# ---- push_scores against push ---------------------------------------------------------------------------------------------
def _scores_of_pushes(torch, bank, twin, ro, pushes):
    """Feed ``bank.push_scores`` and ``twin.push`` the same pushes; check scores against ``score_rows`` of the twin's rows and
    return every stream's concatenated (logits, labels)."""
    n = bank.n_streams
    got = [([], []) for _ in range(n)]
    for args in pushes:
        logits, labels, counts = bank.push_scores(*args)
        rows, want_counts = twin.push(*args)
        assert counts.tolist() == want_counts.tolist()
        assert logits.shape[:2] == rows.shape[:2] == labels.shape
        if rows.shape[1]:
            want_logits, want_labels = ro.score_rows(rows)
        for b in range(n):
            c = int(counts[b])
            if c:
                assert logits[b, :c].cpu().numpy().tobytes() == want_logits[b, :c].cpu().numpy().tobytes()
                assert labels[b, :c].cpu().numpy().tobytes() == want_labels[b, :c].cpu().numpy().tobytes()
            assert not logits[b, c:].any() and (labels[b, c:] == -1).all()
            got[b][0].append(logits[b, :c].cpu().numpy())
            got[b][1].append(labels[b, :c].cpu().numpy())
    return [(np.concatenate(lg), np.concatenate(lb)) for lg, lb in got]


def test_stream_bank_push_scores(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import pipeline, synth
    net, _ = _records(torch)
    S, K, H, G = 8, 3, 1, 12
    model, ro = _readout(5, 70, 12, seed=21, keys=KEYS5)
    raster = synth.bernoulli_raster(3, 24, G * S, 0.25, seed=5)

    def banks():
        return (pipeline.StreamBank(net, 3, S, K, H, KEYS5, readout=ro), pipeline.StreamBank(net, 3, S, K, H, KEYS5))

    whole = _scores_of_pushes(torch, *banks(), ro, [(raster, [G, G, G])])
    assert all(lg.shape == (G - K + 1, 12) and (lb >= 0).all() for lg, lb in whole)
    # cut anywhere, the streams at different places: stream b's segments [done_b, done_b + new_b)
    done = np.zeros(3, dtype=np.int64)
    pushes = []
    for new in ([1, 0, 5], [1, 4, 0], [0, 0, 0], [4, 3, 2], [6, 5, 5]):
        new = np.array(new)
        chunk = np.zeros((3, 24, int(max(new.max(), 1)) * S), dtype=np.uint8)
        for b in range(3):
            chunk[b, :, :new[b] * S] = raster[b, :, done[b] * S:(done[b] + new[b]) * S]
        pushes.append((chunk, new))
        done += new
    assert done.tolist() == [G] * 3
    cut = _scores_of_pushes(torch, *banks(), ro, pushes)
    for b in range(3):
        assert cut[b][0].tobytes() == whole[b][0].tobytes() and cut[b][1].tobytes() == whole[b][1].tobytes(), f"stream {b}"
    with pytest.raises(ValueError, match="needs a readout"):
        pipeline.StreamBank(net, 3, S, K, H, KEYS5).push_scores(raster, [G, G, G])
    with pytest.raises(ValueError, match="the readout was fitted on"):
        pipeline.StreamBank(net, 3, S, K, H, KEYS8, readout=ro)


@pytest.mark.parametrize("kind", ["gammatone", "mel"])
def test_audio_stream_bank_push_scores(torch_cuda, kind):
    """A few hundred ms of synthetic audio in 3 streams: the scores of ragged pushes equal score_rows over a twin bank's rows
    and, concatenated, the scores of the uncut run."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn
    F, S, K, H, hop, hops, n = 24, 8, 3, 1, 160, 40, 3
    rng = np.random.RandomState(77)
    t = np.arange(hops * hop) / (hops * hop)
    audio = np.stack([(rng.standard_normal(hops * hop) * 0.3 * 10.0 ** (-2.5 * np.abs(t - peak))).astype(np.float32)
                      for peak in (0.5, 0.35, 0.65)])
    make = frontend.GammatoneStream if kind == "gammatone" else frontend.MelStream
    # calibrate the fixed dB range on the device's own dB columns
    probe = make(F, n, (-60.0, -10.0)).push(audio, want_db=True)
    db = probe[2].cpu().numpy()[:, :, :int(probe[1].min())]
    lo, hi = (float(v) for v in np.percentile(db[np.isfinite(db)], (20, 80)))
    res = R.build_reservoir(R.SimulationParams(num_neurons=200, num_output_neurons=70, small_world_graph_k=40,
                                               mean_weight=0.3, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    model, ro = _readout(5, 70, 12, seed=31, keys=KEYS5)

    def banks():
        return (pipeline.AudioStreamBank(make(F, n, (lo, hi)), net, S, K, H, KEYS5, readout=ro),
                pipeline.AudioStreamBank(make(F, n, (lo, hi)), net, S, K, H, KEYS5))

    whole = _scores_of_pushes(torch, *banks(), ro, [(audio, None)])
    assert all(len(lb) >= 8 and (lb >= 0).all() for _, lb in whole)
    assert len({lg.tobytes() for lg, _ in whole}) == n and all(len({r.tobytes() for r in lg}) > 1 for lg, _ in whole)
    done = np.zeros(n, dtype=np.int64)
    pushes = []
    for new in ([3, 0, 7], [1, 9, 0], [0, 0, 0], [16, 11, 13], [20, 20, 20]):
        new = np.array(new)
        chunk = np.full((n, int(max(new.max(), 1)) * hop), 7.0, dtype=np.float32)
        for b in range(n):
            chunk[b, :new[b] * hop] = audio[b, done[b] * hop:(done[b] + new[b]) * hop]
        pushes.append((chunk, new))
        done += new
    assert done.tolist() == [hops] * n
    cut = _scores_of_pushes(torch, *banks(), ro, pushes)
    for b in range(n):
        assert cut[b][0].tobytes() == whole[b][0].tobytes() and cut[b][1].tobytes() == whole[b][1].tobytes(), f"stream {b}"
    with pytest.raises(ValueError, match="needs a readout"):
        banks()[1].push_scores(audio)


# ---- capture and replay -----------------------------------------------------------------------------------------------------
def test_both_launches_capture_into_a_graph_and_replay(torch_cuda):
    """One launch of each, no parallel branches: captured, replayed on new inputs, equal to the eager launches."""
    torch = torch_cuda
    net, records = _records(torch)
    model, ro = _readout(5, 70, 12, seed=41, keys=KEYS5)
    x0 = torch.from_numpy(make_case(5, 5, 70, 12, seed=1)[0]).cuda()
    x1 = torch.from_numpy(make_case(5, 5, 70, 12, seed=2)[0]).cuda()
    seg0 = torch.tensor([6, 2, 0], dtype=torch.int32, device="cuda")
    seg1 = torch.tensor([3, 6, 5], dtype=torch.int32, device="cuda")
    eager = [ro.score_rows(x0), ro.score_rows(x1), ro.score_windows(net, records, 8, 3, 1, segments=seg0),
             ro.score_windows(net, records, 8, 3, 1, segments=seg1)]
    torch.cuda.synchronize()
    static_x, static_seg = x0.clone(), seg0.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # capture: any allocation/sync/attribute call would fail it
        rows_out = ro.score_rows(static_x)
        windows_out = ro.score_windows(net, records, 8, 3, 1, segments=static_seg)
    for x, seg, want_rows, want_windows in ((x0, seg0, eager[0], eager[2]), (x1, seg1, eager[1], eager[3]),
                                            (x1, seg1, eager[1], eager[3])):
        static_x.copy_(x)
        static_seg.copy_(seg)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(rows_out + windows_out, want_rows + want_windows):
            assert torch.equal(got, want)
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[2][0], eager[3][0])


# ---- end to end on the synthetic corpus -------------------------------------------------------------------------------------
def test_a_saved_model_rebuilds_the_pipeline_and_labels_as_the_readout_does(torch_cuda, tmp_path, monkeypatch, capsys):
    """Train through main_from_audio(readout="torch-ridge", model_out=...) on 6 clips of each of 12 synthetic classes; load the
    file, rebuild front end and reservoir from its parameters alone: the feature rows are the training run's byte for byte,
    and the device labels are RidgeReadout.predict's wherever its top-two margin exceeds what two summation orders can differ
    by (twice the bound of tests/readout_restatement.py: either logit may move by it).  At most 2 % of the clips may lie under
    that margin.  Then classify.py's two routes run on wav files written from the corpus."""
    torch = torch_cuda
    import create_dataset as cd
    import extract_lsm_features as ex
    import classify
    from lsm_speech_classifier_amd import pipeline, readout
    monkeypatch.chdir(tmp_path)
    words = [f"word{i}" for i in range(12)]
    audio, labels = cd.collect_audio(commands=words, synthetic_per_class=6)
    seen = []
    original = pipeline.features_from_audio

    def recording(clips, *args, **kw):
        rows = original(clips, *args, **kw)
        seen.append((np.array(clips, copy=True), rows.clone()))
        return rows

    monkeypatch.setattr(pipeline, "features_from_audio", recording)
    acc = ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, num_neurons=200, num_output_neurons=80,
                             small_world_k=40, readout="torch-ridge", class_names=words, model_out="kws.npz")
    monkeypatch.setattr(pipeline, "features_from_audio", original)
    assert "Model saved to 'kws.npz'" in capsys.readouterr().out and acc is not None and len(seen) == 2
    model = readout.LinearModel.load("kws.npz")
    assert model.class_names == words and model.n_out == 80 and model.feature_keys == ex.FEATURE_SETS["original"]
    fe, net = pipeline.pipeline_from_params(model.params)
    ro = readout.DeviceReadout(model, net.device)
    clips = np.concatenate([c for c, _ in seen])
    want_rows = torch.cat([r for _, r in seen])
    rows = pipeline.features_from_audio(clips, fe, net, model.feature_keys, device_out=True)
    assert len(clips) == len(audio) == 72 and want_rows.any()
    assert rows.cpu().numpy().tobytes() == want_rows.cpu().numpy().tobytes()
    logits, got = ro.score_rows(rows)
    # the reference: StandardScaler.transform in float64, then RidgeReadout.decision_function, from the file's arrays
    scaler, clf = readout.StandardScaler(), readout.RidgeReadout(1.0)
    scaler.mean_, scaler.scale_ = torch.from_numpy(model.mean), torch.from_numpy(model.scale)
    clf.coef_, clf.intercept_, clf.classes_ = (torch.from_numpy(model.coef), torch.from_numpy(model.intercept),
                                               torch.from_numpy(model.classes))
    x = rows.cpu()
    ref = clf.decision_function(scaler.transform(x.to(torch.float64))).numpy()
    bound = RR.summation_bound(x.numpy(), model.mean, model.scale, model.coef, model.intercept)
    assert (np.abs(logits.cpu().numpy() - ref) <= bound).all()
    top = np.sort(ref, axis=1)
    clear = top[:, -1] - top[:, -2] > 2.0 * bound.max(axis=1)
    print(f"clips under the margin: {(~clear).sum()} of {len(clear)}; largest bound {bound.max():.3g}, "
          f"smallest margin {(top[:, -1] - top[:, -2]).min():.3g}")
    assert (~clear).mean() <= 0.02
    want = clf.predict(scaler.transform(x.to(torch.float64))).numpy()
    assert (ro.class_of(got).cpu().numpy()[clear] == want[clear]).all() and (got.cpu().numpy() >= 0).all()
    assert len(set(want.tolist())) >= 6                                 # a readout that tells the classes apart
    # classify.py on wav files of the corpus: a clip file per class of the first three, and one stream of four clips
    from scipy.io import wavfile
    files = []
    for i in (0, 1, 2):
        files.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(files[-1], 16000, clips[i])                       # float32 PCM: decoded to the same samples
    lines = classify.classify_clips(model, files)
    assert [name for name, _, _ in lines] == files
    assert [cls for _, cls, _ in lines] == [words[int(c)] for c in ro.class_of(got).cpu().numpy()[:3]]
    assert all(margin > 0 for _, _, margin in lines)
    wavfile.write(str(tmp_path / "stream.wav"), 16000, clips[:4].reshape(-1))
    events = classify.classify_streams(model, [str(tmp_path / "stream.wav")], 1000.0, 100.0, hold=2, background=-1)
    assert all(name.endswith("stream.wav") and cls in words and 1000.0 <= t <= 4000.0 for name, t, cls in events)
