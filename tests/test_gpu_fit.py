"""The streaming ridge fit on the device (SPEC.md 7, include/lsm_hip_fit.h): every statistic byte for byte against the NumPy
restatement (tests/fit_restatement.py; NaN entries by position) at the edges of the launch's tiles and stages, however the rows
are cut into pushes and with non-finite features; then `pipeline.fit_from_audio` and the "stream-ridge" route end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_restatement as FR  # noqa: E402
from test_fit_host import launch_shape  # noqa: E402
from test_readout_host import KEYS8  # noqa: E402

pytestmark = pytest.mark.gpu

E, R = launch_shape()                                              # tile edge and rows per stage of the kernel as built
INT32_MIN = -2 ** 31
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def make_rows(n, D, C, seed):
    """Features of random sign across 1e-3 .. 1e4 (the order of the sums matters), integers, +-0 and subnormals among them;
    labels in [0, C) with -1, C and INT32_MIN among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-3, 4, (n, D))).astype(np.float32)
    kind = rng.integers(0, 10, (n, D))
    x[kind == 0] = rng.integers(-40, 40, (n, D)).astype(np.float32)[kind == 0]
    x[kind == 1] = 0.0
    x[kind == 2] = -0.0
    x[kind == 3] = (rng.integers(-100, 100, (n, D)) * np.float64(1.4e-45)).astype(np.float32)[kind == 3]
    y = rng.integers(0, C, n).astype(np.int32)
    for at, bad in zip(range(2, n, 5), (-1, C, INT32_MIN, -1, C, INT32_MIN)):
        y[at] = bad
    return x, y


def device_statistics(torch, n_keys, n_out, C, start=None):
    """Statistics on the GPU, initialised as the caller must -- with the sentinel above the Gram's diagonal -- or to ``start``."""
    from lsm_speech_classifier_amd import readout
    stats = readout.RidgeStatistics(KEYS8[:n_keys], n_out, C, "cuda")
    start = start or FR.new_statistics(n_keys * n_out, C, upper=SENTINEL)
    for name, a in start.items():
        getattr(stats, name).copy_(torch.from_numpy(a))
    return stats


def push(torch, stats, x, y):
    stats.push(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    return stats


def assert_equal(stats, want, what=""):
    for name, a in want.items():
        assert FR.same_bytes(getattr(stats, name).cpu().numpy(), a), f"{what}: {name} differs from the restatement"


# ---- 1. the edges of tiles and stages ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes", [1, 12, 64])
@pytest.mark.parametrize("n_keys,n_out", [(1, 1), (1, E - 1), (3, (E - 1) // 3), (1, E), (1, E + 1), (1, 2 * E + 3)])
def test_edge_shapes_equal_the_restatement_byte_for_byte(torch_cuda, n_keys, n_out, n_classes):
    assert (E - 1) % 3 == 0
    D = n_keys * n_out
    for n_rows in (0, 1, R - 1, R + 1, 300):
        x, y = make_rows(n_rows, D, n_classes, seed=D * 1000 + n_rows + n_classes)
        start = FR.new_statistics(D, n_classes, upper=SENTINEL)
        stats = push(torch_cuda, device_statistics(torch_cuda, n_keys, n_out, n_classes), x, y)
        assert_equal(stats, FR.accumulate(start, x, y), f"{n_rows} rows")
        g = stats.gram.cpu().numpy()
        assert (g[np.triu_indices(D, 1)] == SENTINEL).all()         # nothing above the diagonal is ever written
        if n_rows >= R + 1 and n_classes > 1:
            assert 0 < stats.rows < n_rows and np.isfinite(FR.lower(g)).all()


# ---- 2. however the rows are cut ----------------------------------------------------------------------------------------------
def test_one_push_equals_pushes_of_1_7_64_and_228_rows(torch_cuda):
    torch = torch_cuda
    D, C = 2 * E + 3, 12
    x, y = make_rows(300, D, C, seed=5)
    whole = push(torch, device_statistics(torch, 1, D, C), x, y)
    cut = device_statistics(torch, 1, D, C)
    at = 0
    for n in (1, 7, 64, 228):
        push(torch, cut, x[at:at + n], y[at:at + n])
        at += n
    assert at == 300
    for name in ("gram", "class_sums", "class_counts", "col_min", "col_max"):
        assert getattr(whole, name).cpu().numpy().tobytes() == getattr(cut, name).cpu().numpy().tobytes(), name
    assert_equal(whole, FR.accumulate(FR.new_statistics(D, C, upper=SENTINEL), x, y))
    # and not the bytes of another order: the values are such that the order matters
    back = push(torch, device_statistics(torch, 1, D, C), x[::-1].copy(), y[::-1].copy())
    assert back.gram.cpu().numpy().tobytes() != whole.gram.cpu().numpy().tobytes()


# ---- 3. non-finite features ---------------------------------------------------------------------------------------------------
def test_a_nan_and_an_inf_poison_what_the_definition_says(torch_cuda):
    torch = torch_cuda
    D, C = E + 9, 4
    rng = np.random.default_rng(9)
    x = (rng.uniform(0.5, 2.0, (40, D)) * rng.choice([-1.0, 1.0], (40, D))).astype(np.float32)     # no zero: inf * 0 stays out
    y = (np.arange(40) % C).astype(np.int32)
    x[7, 3], x[21, E + 2] = np.nan, np.inf
    x[30, 5], y[30] = np.nan, -1                                   # a skipped row poisons nothing
    stats = push(torch, device_statistics(torch, 1, D, C), x, y)
    assert_equal(stats, FR.accumulate(FR.new_statistics(D, C, upper=SENTINEL), x, y))
    g = stats.gram.cpu().numpy()
    low = np.tril(np.ones((D, D), bool))
    poisoned = np.zeros((D, D), bool)
    poisoned[3, :] = poisoned[:, 3] = True
    assert (np.isnan(g[low & poisoned])).all() and not np.isnan(g[low & ~poisoned]).any()
    infinite = np.zeros((D, D), bool)
    infinite[E + 2, :] = infinite[:, E + 2] = True
    assert np.isinf(g[low & infinite & ~poisoned]).all() and np.isfinite(g[low & ~infinite & ~poisoned]).all()
    sums = stats.class_sums.cpu().numpy()
    assert np.isnan(sums[7 % C, 3]) and np.isnan(sums).sum() == 1 and sums[21 % C, E + 2] == np.inf and np.isinf(sums).sum() == 1
    mn, mx = stats.col_min.cpu().numpy(), stats.col_max.cpu().numpy()
    kept = np.ones(40, bool)
    kept[30] = False
    rows3 = kept.copy()
    rows3[7] = False
    assert not np.isnan(mn).any() and not np.isnan(mx).any()        # a NaN is never taken
    assert mn[3] == x[rows3, 3].min() and mx[3] == x[rows3, 3].max() and mx[E + 2] == np.inf
    assert mn[5] == x[kept, 5].min() and stats.class_counts.cpu().numpy().tolist() == [10, 10, 9, 10]


# ---- 4. cfg2's row width ------------------------------------------------------------------------------------------------------
def test_the_row_width_of_cfg2_in_one_push(torch_cuda):
    torch = torch_cuda
    x, y = make_rows(256, 2000, 12, seed=2)
    stats = push(torch, device_statistics(torch, 5, 400, 12), x, y)
    assert_equal(stats, FR.accumulate(FR.new_statistics(2000, 12, upper=SENTINEL), x, y))


# ---- 5. end to end on the synthetic corpus ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(torch_cuda):
    """6 clips of each of 12 synthetic classes, a front end and a reservoir for them, and `features_from_audio`'s rows."""
    import create_dataset as cd
    import extract_lsm_features as ex
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as Rv, snn
    words = [f"word{i}" for i in range(12)]
    audio, labels = cd.collect_audio(commands=words, synthetic_per_class=6)
    audio, labels = np.ascontiguousarray(audio, dtype=np.float32), np.asarray(labels, dtype=np.int32)
    fe = frontend.SpikeFrontEnd(32, "gammatone")
    net = snn.SNN(None, reservoir=Rv.build_reservoir(Rv.SimulationParams(
        num_neurons=200, num_output_neurons=80, small_world_graph_k=40, mean_weight=0.3, refractory_period=2), fe.n_channels))
    keys = ex.FEATURE_SETS["original"]
    rows = pipeline.features_from_audio(audio, fe, net, keys, batch=16, device_out=True)
    return words, audio, labels, fe, net, keys, rows


def test_fit_from_audio_gives_the_statistics_of_the_rows_at_any_batch_size(torch_cuda, corpus):
    torch = torch_cuda
    from lsm_speech_classifier_amd import pipeline, readout
    words, audio, labels, fe, net, keys, rows = corpus
    assert len(audio) == 72 and rows.shape == (72, 400) and rows.any()
    fitted = []
    for batch in (16, 72):
        stats = readout.RidgeStatistics(keys, 80, 12, net.device)
        assert pipeline.fit_from_audio(audio, labels, fe, net, keys, stats, batch=batch) == 72
        fitted.append(stats)
    for name in ("gram", "class_sums", "class_counts", "col_min", "col_max"):
        assert getattr(fitted[0], name).cpu().numpy().tobytes() == getattr(fitted[1], name).cpu().numpy().tobytes(), name
    assert_equal(fitted[0], FR.accumulate(FR.new_statistics(400, 12), rows.cpu().numpy(), labels))
    assert fitted[0].rows == 72
    # the readout solved from the statistics labels the clips as the stored-rows fit does
    s = fitted[0].solve(1.0)
    x64 = rows.to(torch.float64)
    got = (((x64 - s.mean) / s.scale) @ s.coef.T + s.intercept).argmax(dim=1)
    scaler = readout.StandardScaler().fit(rows)
    z = scaler.transform(x64)
    clf = readout.RidgeReadout(1.0).fit(z, torch.from_numpy(labels).to(rows.device))
    want = clf.predict(z)
    assert torch.equal(s.classes[got], want.to(torch.int64)) and len(set(want.tolist())) >= 6
    with pytest.raises(ValueError, match="one value per clip"):
        pipeline.fit_from_audio(audio, labels[:-1], fe, net, keys, fitted[0])
    with pytest.raises(ValueError, match="statistics hold rows"):
        pipeline.fit_from_audio(audio, labels, fe, net, keys[:2], fitted[0])


def test_the_stream_ridge_route_writes_a_model_and_two_epochs_double_the_counts(torch_cuda, corpus, tmp_path, monkeypatch,
                                                                                capsys):
    torch = torch_cuda
    import create_dataset as cd
    import extract_lsm_features as ex
    from lsm_speech_classifier_amd import pipeline, readout
    words, audio, labels = corpus[:3]
    monkeypatch.chdir(tmp_path)
    kw = dict(num_neurons=200, num_output_neurons=80, small_world_k=40, class_names=words)
    acc = ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="stream-ridge", model_out="kws.npz", **kw)
    out = capsys.readouterr().out
    assert acc is not None and "is not written on this route" in out and "Model saved to 'kws.npz'" in out
    assert "statistics of 57 training rows" in out and not os.path.exists(ex.FEATURE_FILE)
    model = readout.LinearModel.load("kws.npz")
    assert model.class_names == words and model.n_out == 80 and model.feature_keys == ex.FEATURE_SETS["original"]
    fe, net = pipeline.pipeline_from_params(model.params)
    scorer = readout.DeviceReadout(model, net.device)
    labels_out = scorer.score_rows(pipeline.features_from_audio(audio, fe, net, model.feature_keys, device_out=True))[1]
    assert (labels_out.cpu().numpy() >= 0).all() and len(set(labels_out.cpu().numpy().tolist())) >= 6
    # the same rows as "torch-ridge" sees: the same test predictions, so the same accuracy
    assert acc == ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="torch-ridge", **kw)
    capsys.readouterr()
    # two epochs with a noise plan: every class count doubles, and the second epoch's rows are other rows
    augment = dict(noise_dir="synthetic", snr_db=(5.0, 20.0), time_shift_ms=50.0, level_db=0.0, seed=42)
    corrupt = cd.corruption(augment, len(audio))
    seen = []
    original = pipeline.fit_from_audio

    def recording(clips, y, fe_, net_, keys_, stats, **kw_):
        before = stats.class_counts.cpu().numpy().copy()
        n = original(clips, y, fe_, net_, keys_, stats, **kw_)
        seen.append((before, stats.class_counts.cpu().numpy().copy(), stats.class_sums.cpu().numpy().copy(), kw_["corrupt"][1]))
        return n

    monkeypatch.setattr(pipeline, "fit_from_audio", recording)
    ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="stream-ridge", epochs=2, corrupt=corrupt,
                       epoch_plans=lambda e: cd.epoch_plans(e, len(audio), augment, corrupt), **kw)
    assert "statistics of 114 training rows" in capsys.readouterr().out and len(seen) == 2
    (zero, once, sums_once, plan0), (_, twice, sums_twice, plan1) = seen
    assert not zero.any() and once.sum() == 57 and (twice == 2 * once).all()
    assert not np.array_equal(np.asarray(plan0.offsets), np.asarray(plan1.offsets))
    assert not np.allclose(sums_twice, 2 * sums_once, rtol=1e-9)
