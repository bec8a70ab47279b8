"""The model-file flags of the scripts (SPEC.md 6), CPU only: --model-out of extract_lsm_features.py and train_classifier.py,
--save-model of main.py, classify.py's own flags and helpers.  Without the new flags the commands main.py starts, File 2 and
everything the stages print are what they were; tests/test_script_flags.py, which pins the older flags, is not touched."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_restatement as RR  # noqa: E402

KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']


@pytest.mark.parametrize("script,flags", [
    ("extract_lsm_features.py", ["--model-out", "--filterbank", "--n-filters"]),
    ("train_classifier.py", ["--model-out"]),
    ("main.py", ["--save-model"]),
    ("classify.py", ["--model", "--stream", "--window-ms", "--hop-ms", "--hold", "--background"]),
])
def test_the_new_flags_are_offered(script, flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for f in flags:
        assert f in out.stdout, f"{script} lacks {f}"


def test_extract_refuses_model_out_without_its_front_end_or_with_time_segments():
    import extract_lsm_features as ex
    r = subprocess.run([sys.executable, os.path.join(ROOT, "extract_lsm_features.py"), "--model-out", "m.npz"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--model-out needs --filterbank and --n-filters" in r.stderr
    with pytest.raises(ValueError, match="--model-out needs --filterbank"):
        ex.main("original", 0.6, model_out="m.npz")
    with pytest.raises(ValueError, match="--model-out needs --time-segments 1"):
        ex.main("original", 0.6, time_segments=4, model_out="m.npz", front_end=("gammatone", 32))
    ex.check_model_out(None, 4)
    ex.check_model_out("m.npz", 1)


def test_main_forwards_save_model_and_nothing_without_it(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert [c[1:] for c in calls] == [
        [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"],
        [os.path.join(ROOT, "extract_lsm_features.py"), "--feature-set", "original", "--multiplier", "0.6"],
        [os.path.join(ROOT, "train_classifier.py")]]
    calls.clear()
    pipeline.run_pipeline(64, "mel", "all", 0.6, save_model="kws.npz", readout="torch-ridge")
    s1, s2, s3 = calls
    assert "kws.npz" not in s1
    assert s2[2:] == ["--feature-set", "all", "--multiplier", "0.6", "--model-out", "kws.npz", "--filterbank", "mel",
                      "--n-filters", "64"]
    assert s3[2:] == ["--readout", "torch-ridge", "--model-out", "kws.npz"]
    calls.clear()
    # the in-memory route: the one process gets the path; with a PyTorch readout there is no stage 3
    pipeline.run_pipeline(64, "mel", "all", 0.6, in_memory=True, save_model="kws.npz", readout="torch-ridge")
    assert len(calls) == 1 and "'save_model': 'kws.npz'" in calls[0][2] and '"model_out": a.save_model' in calls[0][2]
    compile(calls[0][2], "<in-memory>", "exec")
    calls.clear()
    pipeline.run_pipeline(64, "mel", "all", 0.6, in_memory=True, save_model="kws.npz")
    assert len(calls) == 2 and calls[1][2:] == ["--model-out", "kws.npz"]
    calls.clear()
    pipeline.run_pipeline(64, "mel", "all", 0.6, in_memory=True)
    assert "'save_model': None" in calls[0][2] and calls[1][2:] == []


def _rows(seed=3, n=60, n_out=6, n_classes=3):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % n_classes
    centres = rng.standard_normal((n_classes, len(KEYS) * n_out)) * 4.0
    x = (centres[y] + rng.standard_normal((n, len(KEYS) * n_out))).astype(np.float32)
    x[:, 5] = 0.0                                                       # a column without variance: scale 1
    return x, y.astype(np.int32)


def _params():
    return dict(filterbank="gammatone", n_filters=32, redundancy=1, thresholds=[0.7, 0.8, 0.9, 0.95], gap=0.1, time_bins=100,
                n_samples=16000, n_channels=32, num_neurons=200, num_output_neurons=6, mean_weight=0.0123456789012345,
                weight_variance=10, membrane_threshold=2.0, leak_coefficient=0.01, refractory_period=2,
                small_world_graph_p=0.1, small_world_graph_k=40, seed=42, leak_variance_divisor=None,
                feature_set="original", multiplier=0.6, time_segments=1)


def test_the_device_readout_route_writes_the_whole_model_and_leaves_file_2_and_the_report_alone(tmp_path, monkeypatch):
    """extract_lsm_features._device_readout on CPU tensors (the code main_from_audio(readout="torch-ridge") ends in)."""
    import torch
    import extract_lsm_features as ex
    from lsm_speech_classifier_amd import readout
    monkeypatch.chdir(tmp_path)
    x, y = _rows()
    xtr, xte, ytr, yte = torch.from_numpy(x[:45]), torch.from_numpy(x[45:]), y[:45], y[45:]
    names = ["go", "stop", "wait"]

    def run(model_file):
        out = io.StringIO()
        with redirect_stdout(out):
            acc = ex._device_readout(xtr, xte, ytr, yte, "torch-ridge", "original", None, names, model_file)
        with np.load(ex.FEATURE_FILE, allow_pickle=True) as f:
            return acc, out.getvalue(), {k: f[k].tobytes() for k in f.files}

    acc0, text0, file0 = run(None)
    acc1, text1, file1 = run(dict(path="kws.npz", feature_keys=KEYS, n_out=6, params=_params()))
    assert acc0 == acc1 and file0 == file1
    assert sorted(file0) == ["X_test_features", "X_train_features", "feature_set", "leak_variance_divisor", "y_test", "y_train"]
    assert text1 == text0.replace("\n\n--- Final Results", "\nModel saved to 'kws.npz'\n\n--- Final Results") != text0
    m = readout.LinearModel.load("kws.npz")
    assert m.class_names == names and m.classes.tolist() == [0, 1, 2] and m.feature_keys == KEYS and m.n_out == 6
    assert m.params == _params() and m.scale[5] == 1.0
    # the saved model predicts what the readout predicted
    scaler = readout.StandardScaler().fit(xtr)
    clf = readout.RidgeReadout(1.0).fit(scaler.transform(xtr), torch.from_numpy(ytr))
    logits, labels = RR.scores(x[45:], m.mean, m.scale, m.coef, m.intercept, len(KEYS), 6)
    assert (m.classes[labels] == clf.predict(scaler.transform(xte)).numpy()).all() and (labels == yte).mean() > 0.9


def test_train_classifier_completes_the_front_half_and_prints_what_it_printed(tmp_path, monkeypatch):
    import train_classifier as tc
    from sklearn.preprocessing import StandardScaler
    from lsm_speech_classifier_amd import readout
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LSM_READOUT", raising=False)
    x, y = _rows(seed=5)
    scaler = StandardScaler().fit(x[:45].astype(np.float64))
    np.savez_compressed(tc.FEATURE_FILE, X_train_features=scaler.transform(x[:45]), y_train=y[:45],
                        X_test_features=scaler.transform(x[45:]), y_test=y[45:], feature_set="original",
                        leak_variance_divisor=None)
    import extract_lsm_features as ex
    with redirect_stdout(io.StringIO()):
        ex.write_model_front(scaler, "kws.npz", KEYS, 6, _params())
    with pytest.raises(ValueError, match="front half"):
        readout.LinearModel.load("kws.npz")

    def run(**kw):
        out = io.StringIO()
        with redirect_stdout(out):
            acc = tc.train_and_evaluate_classifier(class_names=["go", "stop", "wait"], **kw)
        return acc, out.getvalue()

    acc0, text0 = run()
    for kind in ("sklearn", "torch-ridge"):
        with redirect_stdout(io.StringIO()):
            ex.write_model_front(scaler, "kws.npz", KEYS, 6, _params())
        acc1, text1 = run(readout=kind, model_out="kws.npz")
        if kind == "sklearn":
            assert acc1 == acc0 and text1 == text0.replace("\n\n--- Final Results", "\nModel saved to 'kws.npz'\n\n--- Final Results")
        m = readout.LinearModel.load("kws.npz")
        assert m.coef.shape == (3, 30) and m.class_names == ["go", "stop", "wait"] and m.params == _params()
        assert m.mean.tobytes() == scaler.mean_.tobytes() and m.scale.tobytes() == scaler.scale_.tobytes()
        _, labels = RR.scores(x[45:], m.mean, m.scale, m.coef, m.intercept, len(KEYS), 6)
        assert (m.classes[labels] == y[45:]).mean() > 0.9
    assert "Model file not found" in run(model_out="absent.npz")[1]


def test_classify_helpers():
    import classify
    assert classify.window_plan(1000.0, 100.0, 4) == (40, 10, 1)
    assert classify.window_plan(1000.0, 10.0, 4) == (4, 100, 1)
    assert classify.window_plan(500.0, 250.0, 4) == (100, 2, 1)
    assert classify.window_plan(300.0, 100.0, 4, segment_steps=8) == (8, 15, 5)
    with pytest.raises(SystemExit):
        classify.window_plan(100.0, 200.0, 4)
    with pytest.raises(SystemExit):
        classify.window_plan(200000.0, 100.0, 4)
    assert classify.top_two_margin(np.array([1.0, 4.5, 3.0])) == 1.5 and classify.top_two_margin(np.array([2.0])) == float("inf")
    assert np.isnan(classify.top_two_margin(np.array([1.0, np.nan])))
    a = classify.build_parser().parse_args(["--model", "m.npz", "a.wav", "b.wav"])
    assert (a.stream, a.window_ms, a.hop_ms, a.hold, a.background, a.files) == (False, 1000.0, 100.0, 3, -1, ["a.wav", "b.wav"])
    a = classify.build_parser().parse_args(["--model", "m.npz", "--stream", "--window-ms", "500", "--hop-ms", "50", "a.wav"])
    assert a.stream and a.window_ms == 500.0 and a.hop_ms == 50.0


def test_model_params_round_trip_through_the_file(tmp_path):
    """pipeline.model_params reads plain attributes: a stand-in front end serves; the dict survives the file unchanged."""
    from types import SimpleNamespace
    from lsm_speech_classifier_amd import pipeline, readout
    from lsm_speech_classifier_amd.reservoir import SimulationParams
    fe = SimpleNamespace(filterbank="mel", n_filters=40, redundancy=2, thresholds=[0.7, 0.8, 0.9, 0.95], gap=0.1, time_bins=100,
                         n_samples=16000, n_channels=80)
    sim = SimulationParams(num_neurons=500, num_output_neurons=200, small_world_graph_k=100, leak_variance_divisor=4)
    sim.mean_weight = np.float64(0.6) * 0.0123456789
    sim.weight_variance = 10
    p = pipeline.model_params(fe, sim, feature_set="all", multiplier=0.6, time_segments=1)
    m = readout.LinearModel(np.zeros(5), np.ones(5), np.zeros((2, 5)), np.zeros(2), [0, 1], ["spike_counts"], 5, params=p)
    m.save(str(tmp_path / "m.npz"))
    back = readout.LinearModel.load(str(tmp_path / "m.npz")).params
    assert back == p and back["mean_weight"] == float(sim.mean_weight) and back["leak_variance_divisor"] == 4.0
    assert set(p) >= {"filterbank", "n_filters", "thresholds", "gap", "redundancy", "time_bins", "n_samples", "num_neurons",
                      "num_output_neurons", "small_world_graph_k", "small_world_graph_p", "seed", "leak_coefficient",
                      "leak_variance_divisor", "mean_weight", "weight_variance", "membrane_threshold", "refractory_period",
                      "time_segments"}
