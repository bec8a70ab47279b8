"""The streaming ridge fit (SPEC.md 7, include/lsm_hip_fit.h), what can be checked without a GPU: header, binding and build
lists, the launch's refusals (made before any device work), `readout.RidgeStatistics` -- `solve` against the stored-rows fit
on statistics the NumPy restatement (tests/fit_restatement.py) makes, `merge`, the file, the rank-order merge over gloo -- and
the scripts' flags."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_restatement as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("lsm_fit_supported", "lsm_fit_accumulate_f32")
KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']


# ---- header, binding, build -------------------------------------------------------------------------------------------------
def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_binding_and_library_carry_the_two_names(tmp_path):
    import shutil
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_fit.h")).read()
    assert _params(header, "lsm_fit_supported") == ["int n_keys", "int n_out", "int n_classes"]
    assert _params(header, "lsm_fit_accumulate_f32") == [
        "const float *features", "const int32_t *labels", "int n_rows", "int n_keys", "int n_out", "int n_classes",
        "double *gram", "double *class_sums", "int64_t *class_counts", "float *col_min", "float *col_max", "void *stream"]
    assert _lib.FIT_SYMBOLS == tuple(_lib.FIT_SIGS) == NEW
    for name in NEW:
        res, args = _lib.FIT_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params)
        for p, ctype in zip(params, args):
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    older = [_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
             _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS, _lib.RAGGED_SIGS, _lib.STEP_SIGS,
             _lib.STEP_STATE_SIGS, _lib.TRIM_SIGS, _lib.RAGGED_AUGMENT_SIGS]
    assert sum(len(t) for t in older) == 83 and len(set().union(*older)) == 83      # the older tables keep their sizes
    assert len(_lib.READOUT_SIGS) == 3 and not set(NEW) & (set().union(*older) | set(_lib.READOUT_SIGS))
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert "fit.hip" in build.SOURCES and "lsm_hip_fit.h" in build.ABI_HEADERS
    assert "lsm_hip_readout.h" in build.ABI_HEADERS and len(build.PUBLIC_HEADERS) == 9
    # the header is hashed into the build id: another text of it, another id
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(include_dir=str(inc)) == build.source_id()
    with open(inc / "lsm_hip_fit.h", "a") as f:
        f.write("/* changed */\n")
    assert build.source_id(include_dir=str(inc)) != build.source_id()


def launch_shape():
    """(tile edge, rows per stage) of the launch as built, as the public header states them."""
    header = open(os.path.join(ROOT, "include", "lsm_hip_fit.h")).read()
    return (int(re.search(r"^#define LSM_FIT_TILE (\d+)$", header, re.M).group(1)),
            int(re.search(r"^#define LSM_FIT_STAGE_ROWS (\d+)$", header, re.M).group(1)))


def test_the_header_states_the_shape_the_kernel_is_built_with():
    source = open(os.path.join(ROOT, "lsm-speech-classifier_amd", "csrc", "fit.hip")).read()
    m = re.search(r"^constexpr int TILE = (\d+), STAGE = (\d+);", source, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == launch_shape()


def test_supported_sizes():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    for good in ((1, 1, 1), (8, 2048, 64), (1, 16384, 1), (5, 3200, 12), (8, 2000, 35)):
        assert lib.lsm_fit_supported(*good) == 1, good
    for bad in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 16385, 1), (8, 2049, 1), (5, 3277, 1), (1, 1, 0), (1, 1, 65),
                (8, 2 ** 29, 1)):
        assert lib.lsm_fit_supported(*bad) == 0, bad


X, Y, G, S, N, MN, MX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def _in_order(call, later, texts):
    """Each row breaks its own rule AND every later one: the message names the earliest."""
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)


def test_refusals_in_their_order():
    """Every refusal is made on the host before anything is launched, so fake (aligned, distinct) addresses serve."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    good = dict(features=X, labels=Y, n_rows=3, n_keys=5, n_out=70, n_classes=12, gram=G, class_sums=S, class_counts=N,
                col_min=MN, col_max=MX)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_fit_accumulate_f32(a["features"] or None, a["labels"] or None, a["n_rows"], a["n_keys"], a["n_out"],
                                        a["n_classes"], a["gram"] or None, a["class_sums"] or None, a["class_counts"] or None,
                                        a["col_min"] or None, a["col_max"] or None, None)
        return rc, lib.lsm_last_error().decode()

    later = [dict(n_rows=-1), dict(n_keys=9), dict(n_out=0), dict(n_classes=65), dict(col_max=0)]
    texts = ["n_rows=-1", "n_keys=9", "n_out=0", "n_classes=65", "are required"]
    _in_order(call, later, texts)
    # D is judged between n_out and n_classes
    _in_order(call, [dict(n_keys=8, n_out=2049), dict(n_classes=0), dict(gram=0)], ["D = n_keys * n_out = 16392", "n_classes=0",
                                                                                     "are required"])
    # a pointer that is NULL cannot also be misaligned: the alignment rules in their own run
    _in_order(call, [dict(class_sums=S + 4), dict(labels=Y + 2)], ["8-byte aligned", "4-byte aligned"])
    for kw, text in ((dict(n_keys=0), "n_keys=0"), (dict(n_out=-3), "n_out=-3"), (dict(n_keys=1, n_out=16385), "D = n_keys"),
                     (dict(n_classes=0), "n_classes=0"), (dict(gram=0), "are required"), (dict(class_sums=0), "are required"),
                     (dict(class_counts=0), "are required"), (dict(col_min=0), "are required"),
                     (dict(gram=G + 4), "8-byte aligned"), (dict(class_counts=N + 4), "8-byte aligned"),
                     (dict(features=X + 2), "4-byte aligned"), (dict(col_min=MN + 1), "4-byte aligned"),
                     (dict(col_max=MX + 2), "4-byte aligned"), (dict(features=0), "null features or labels"),
                     (dict(labels=0), "null features or labels")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert call(n_rows=0)[0] == 0 and call(n_rows=0, features=0, labels=0)[0] == 0      # nothing to do, nothing launched
    assert call(n_keys=1, n_out=16384, n_rows=0)[0] == 0


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_definition_and_is_cut_invariant():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((40, 9)) * 10.0 ** rng.integers(-3, 5, (40, 9))).astype(np.float32)
    y = rng.integers(-1, 4, 40).astype(np.int32)                    # -1 and 3 lie outside [0, 3)
    whole = FR.accumulate(FR.new_statistics(9, 3, upper=-7.0), x, y)
    G_ = np.zeros((9, 9))
    for r in range(40):
        if 0 <= y[r] < 3:
            G_ += np.outer(x[r].astype(np.float64), x[r].astype(np.float64))
    assert FR.lower(whole["gram"]).tobytes() == FR.lower(G_).tobytes()
    assert (whole["gram"][np.triu_indices(9, 1)] == -7.0).all()
    kept = (y >= 0) & (y < 3)
    assert whole["class_counts"].tolist() == [int((y == c).sum()) for c in range(3)]
    assert (whole["col_min"] == x[kept].min(axis=0)).all() and (whole["col_max"] == x[kept].max(axis=0)).all()
    cut = FR.new_statistics(9, 3, upper=-7.0)
    for lo, hi in ((0, 1), (1, 8), (8, 8), (8, 40)):
        cut = FR.accumulate(cut, x[lo:hi], y[lo:hi])
    assert all(FR.same_bytes(whole[k], cut[k]) for k in whole)
    x[5, 2], y[5] = np.nan, 1
    nan = FR.accumulate(FR.new_statistics(9, 3), x, y)
    assert np.isnan(nan["gram"][2, :3]).all() and np.isnan(nan["gram"][4, 2]) and not np.isnan(nan["gram"][4, 3])
    assert np.isnan(nan["class_sums"][1, 2]) and not np.isnan(nan["col_min"]).any() and not np.isnan(nan["col_max"]).any()


# ---- RidgeStatistics.solve ---------------------------------------------------------------------------------------------------
# The largest logit difference to the stored-rows fit measured on this input (profiles/ridge_fit.txt); the test allows 100
# times that for the two float64 summation orders, and that bound must stay below 1e-9.
MEASURED_LOGIT_DIFFERENCE = 4.8e-14
ZERO, CONSTANT, SMALL = 17, 60, 133                                 # the all-zero, the constant and the 1e-3 column


def solve_case():
    """n = 600 rows of D = 200 (5 keys x 40), C = 12, ten rows labelled -1: (x, y, the restatement's statistics)."""
    rng = np.random.default_rng(7)
    n, D, C = 600, 200, 12
    y = (np.arange(n) % C).astype(np.int32)
    centres = rng.standard_normal((C, D)) * 3.0 + 6.0
    x = (centres[y] + rng.standard_normal((n, D)) * 2.0).astype(np.float32)
    x[:, ZERO] = 0.0
    x[:, CONSTANT] = np.float32(41.7)
    x[:, SMALL] *= np.float32(1e-3)
    y[rng.choice(n, 10, replace=False)] = -1
    return x, y, FR.accumulate(FR.new_statistics(D, C), x, y)


@pytest.fixture(scope="module")
def solved():
    from lsm_speech_classifier_amd import readout
    x, y, st = solve_case()
    stats = readout.RidgeStatistics.from_arrays(st["gram"], st["class_sums"], st["class_counts"], st["col_min"],
                                                st["col_max"], KEYS, 40)
    return x, y, stats, stats.solve(1.0)


def _logits(x, s):
    return ((x.astype(np.float64) - s.mean.numpy()) / s.scale.numpy()) @ s.coef.numpy().T + s.intercept.numpy()


def test_solve_gives_the_labels_of_the_stored_rows_fit_and_of_scikit_learn(solved):
    import torch
    from sklearn.linear_model import RidgeClassifier
    from sklearn.preprocessing import StandardScaler as SkScaler
    from lsm_speech_classifier_amd import readout
    x, y, stats, s = solved
    kept = y >= 0
    assert stats.rows == 590 and kept.sum() == 590
    assert s.mean.shape == s.scale.shape == (200,) and s.coef.shape == (12, 200) and s.intercept.shape == (12,)
    assert all(t.dtype == torch.float64 and t.device.type == "cpu" for t in (s.mean, s.scale, s.coef, s.intercept))
    assert s.classes.tolist() == list(range(12))
    # the constant columns: their value, scale 1, out of the system
    assert s.mean[CONSTANT].item() == float(np.float32(41.7)) and s.mean[ZERO].item() == 0.0
    assert s.scale[CONSTANT].item() == s.scale[ZERO].item() == 1.0
    assert not s.coef[:, [ZERO, CONSTANT]].any() and s.coef[:, SMALL].abs().min() > 0
    got = _logits(x[kept], s)
    # this package's stored-rows fit
    xt, yt = torch.from_numpy(x[kept]), torch.from_numpy(y[kept])
    scaler = readout.StandardScaler().fit(xt)
    z = scaler.transform(xt.to(torch.float64))
    clf = readout.RidgeReadout(1.0).fit(z, yt)
    ref = clf.decision_function(z).numpy()
    diff = float(np.abs(got - ref).max())
    top = np.sort(ref, axis=1)
    print(f"largest logit difference to the stored-rows fit: {diff:.3e}; smallest top-two margin {np.min(top[:, -1] - top[:, -2]):.3e}")
    bound = 100 * MEASURED_LOGIT_DIFFERENCE
    assert bound < 1e-9 and diff <= bound
    assert (got.argmax(axis=1) == clf.predict(z).numpy()).all()
    assert np.abs(s.scale.numpy() - scaler.scale_.numpy()).max() < 1e-9 and np.abs(s.mean.numpy() - scaler.mean_.numpy()).max() < 1e-9
    # scikit-learn on its own scaler's output
    x64 = x[kept].astype(np.float64)
    sk_scaler = SkScaler().fit(x64)
    sk = RidgeClassifier(alpha=1.0).fit(sk_scaler.transform(x64), y[kept])
    assert (s.classes.numpy()[got.argmax(axis=1)] == sk.predict(sk_scaler.transform(x64))).all()
    assert np.abs(got - sk.decision_function(sk_scaler.transform(x64))).max() <= bound


def test_solve_leaves_out_classes_without_rows_and_refuses_no_rows(solved):
    from lsm_speech_classifier_amd import readout
    x, y, _, _ = solved
    y2 = np.where(y == 4, -1, y).astype(np.int32)
    st = FR.accumulate(FR.new_statistics(200, 12), x, y2)
    stats = readout.RidgeStatistics.from_arrays(st["gram"], st["class_sums"], st["class_counts"], st["col_min"],
                                                st["col_max"], KEYS, 40)
    s = stats.solve(1.0)
    assert s.classes.tolist() == [c for c in range(12) if c != 4] and s.coef.shape == (11, 200)
    model = stats.to_model(0.5, [f"w{c}" for c in range(12)], dict(filterbank="gammatone"))
    assert model.class_names == [f"w{c}" for c in range(12) if c != 4] and model.n_classes == 11 and model.n_out == 40
    assert model.classes.tolist() == s.classes.tolist() and model.params == dict(filterbank="gammatone")
    with pytest.raises(ValueError, match="name all 12"):
        stats.to_model(1.0, ["a"])
    empty = readout.RidgeStatistics(KEYS, 40, 12, device="cpu")
    with pytest.raises(ValueError, match="no rows"):
        empty.solve()
    with pytest.raises(ValueError, match="1 to 64 classes"):
        readout.RidgeStatistics(KEYS, 40, 65, device="cpu")
    with pytest.raises(ValueError, match="gram must have shape"):
        readout.RidgeStatistics.from_arrays(st["gram"][:-1], st["class_sums"], st["class_counts"], st["col_min"],
                                            st["col_max"], KEYS, 40)
    with pytest.raises(Exception, match="GPU|HIP device|no host fallback"):    # push has no host fallback
        import torch
        empty.push(torch.zeros((1, 200)), torch.zeros((1,), dtype=torch.int32))


# ---- merge and the file -----------------------------------------------------------------------------------------------------
def _halves():
    from lsm_speech_classifier_amd import readout
    x, y, _ = solve_case()
    parts = [FR.accumulate(FR.new_statistics(200, 12), x[lo:hi], y[lo:hi]) for lo, hi in ((0, 250), (250, 600))]
    make = lambda st: readout.RidgeStatistics.from_arrays(st["gram"], st["class_sums"], st["class_counts"], st["col_min"],  # noqa: E731
                                                          st["col_max"], KEYS, 40)
    return parts, [make(st) for st in parts]


def test_merge_equals_addition_byte_for_byte():
    from lsm_speech_classifier_amd import readout
    (a, b), (sa, sb) = _halves()
    merged = sa.merge(sb)
    assert merged is sa
    assert FR.lower(merged.gram.numpy()).tobytes() == FR.lower(a["gram"] + b["gram"]).tobytes()
    assert merged.class_sums.numpy().tobytes() == (a["class_sums"] + b["class_sums"]).tobytes()
    assert merged.class_counts.numpy().tobytes() == (a["class_counts"] + b["class_counts"]).tobytes() and merged.rows == 590
    assert merged.col_min.numpy().tobytes() == np.minimum(a["col_min"], b["col_min"]).tobytes()
    assert merged.col_max.numpy().tobytes() == np.maximum(a["col_max"], b["col_max"]).tobytes()
    # defined, and not one uncut run: close to it, different in the last bits
    _, _, whole = solve_case()
    assert merged.class_counts.numpy().tolist() == whole["class_counts"].tolist()
    assert np.allclose(FR.lower(merged.gram.numpy()), FR.lower(whole["gram"]), rtol=1e-12, atol=0)
    assert FR.lower(merged.gram.numpy()).tobytes() != FR.lower(whole["gram"]).tobytes()
    with pytest.raises(ValueError, match="do not merge"):
        sa.merge(readout.RidgeStatistics(KEYS, 40, 11, device="cpu"))


def test_save_and_load_round_trip_every_byte(tmp_path):
    from lsm_speech_classifier_amd import readout
    _, (sa, _) = _halves()
    path = str(tmp_path / "statistics.npz")
    sa.save(path)
    assert os.path.exists(path)                                         # the caller's path, no suffix appended
    with np.load(path, allow_pickle=False) as z:                        # arrays and short strings only, the triangle packed
        assert all(z[k].dtype.kind in "fiU" for k in z.files)
        assert z["gram_tril"].shape == (200 * 201 // 2,) and int(z["rows"]) == sa.rows and int(z["n_classes"]) == 12
        assert int(z["n_out"]) == 40 and [str(k) for k in z["feature_keys"]] == KEYS
    back = readout.RidgeStatistics.load(path)
    assert back.feature_keys == KEYS and back.n_out == 40 and back.n_classes == 12 and back.rows == sa.rows
    assert back.packed_gram().tobytes() == sa.packed_gram().tobytes()
    for name in ("class_sums", "class_counts", "col_min", "col_max"):
        a, b = getattr(sa, name), getattr(back, name)
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), name
    # loaded statistics go on: another merge, the same solve
    assert np.array_equal(back.solve(1.0).coef.numpy(), sa.solve(1.0).coef.numpy())


# ---- the rank-order merge over gloo -----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_the_rank_order_merge_is_identical_on_both_ranks(tmp_path):
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_fit_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    from lsm_speech_classifier_amd import readout
    (_, _), (sa, sb) = _halves()
    want = sa.merge(sb)                                                 # rank 0's, then rank 1's
    for rank in range(2):
        got = readout.RidgeStatistics.load(str(tmp_path / f"rank{rank}.npz"))
        assert got.packed_gram().tobytes() == want.packed_gram().tobytes()
        for name in ("class_sums", "class_counts", "col_min", "col_max"):
            assert getattr(got, name).numpy().tobytes() == getattr(want, name).numpy().tobytes(), (rank, name)


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def test_main_offers_the_flags_and_refuses_them_where_they_do_not_apply(monkeypatch):
    import main as pipeline
    out = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and all(f in out.stdout for f in ("stream-ridge", "--augment-epochs", "--ridge-alpha"))
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    with pytest.raises(SystemExit, match="needs --in-memory"):
        pipeline.run_pipeline(64, "gammatone", "original", 0.6, readout="stream-ridge")
    with pytest.raises(SystemExit, match="need --readout stream-ridge"):
        pipeline.run_pipeline(64, "gammatone", "original", 0.6, in_memory=True, readout="torch-ridge", augment_epochs=2)
    with pytest.raises(SystemExit, match="need --readout stream-ridge"):
        pipeline.run_pipeline(64, "gammatone", "original", 0.6, ridge_alpha=0.5)
    with pytest.raises(SystemExit, match="must be >= 1"):
        pipeline.run_pipeline(64, "gammatone", "original", 0.6, in_memory=True, readout="stream-ridge", augment_epochs=0)
    with pytest.raises(SystemExit, match="--time-segments 1"):
        pipeline.run_pipeline(64, "gammatone", "original", 0.6, in_memory=True, readout="stream-ridge", time_segments=4)
    assert calls == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--readout", "stream-ridge"], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, LSM_IN_MEMORY="0"))
    assert r.returncode != 0 and "needs --in-memory" in r.stderr
    # the route: one process, no stage 3, the passes, the penalty and the later plans in its call
    pipeline.run_pipeline(64, "gammatone", "original", 0.6, in_memory=True, readout="stream-ridge", augment_epochs=3,
                          ridge_alpha=0.25, save_model="kws.npz", noise_dir="synthetic", snr_db="5,20")
    assert len(calls) == 1
    code = calls[0][2]
    compile(code, "<in-memory>", "exec")
    assert "'augment_epochs': 3" in code and "'ridge_alpha': 0.25" in code and "'device_readout': 'stream-ridge'" in code
    assert "epochs=a.augment_epochs" in code and "cd.epoch_plans(e, len(audio)" in code and "'save_model': 'kws.npz'" in code
    calls.clear()
    pipeline.run_pipeline(64, "gammatone", "original", 0.6, in_memory=True, readout="stream-ridge")
    assert "'augment_epochs': 1" in calls[0][2] and "'ridge_alpha': 1.0" in calls[0][2] and len(calls) == 1


def test_commands_without_the_new_flags_are_unchanged(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert [c[1:] for c in calls] == [
        [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"],
        [os.path.join(ROOT, "extract_lsm_features.py"), "--feature-set", "original", "--multiplier", "0.6"],
        [os.path.join(ROOT, "train_classifier.py")]]
    for readout in (None, "torch-ridge"):
        calls.clear()
        pipeline.run_pipeline(64, "mel", "all", 0.6, in_memory=True, readout=readout)
        code = calls[0][2]
        assert not any(word in code for word in ("epochs", "ridge_alpha", "epoch_plans", "stream-ridge")), readout
        assert code.endswith('**({"model_out": a.save_model} if a.save_model else {}))\n')
        assert len(calls) == (1 if readout else 2)


def test_main_from_audio_refusals_come_before_any_work():
    import extract_lsm_features as ex
    audio, labels = np.zeros((4, 16000), np.float32), np.arange(4)
    with pytest.raises(ValueError, match="epochs needs readout='stream-ridge'"):
        ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="torch-ridge", epochs=2)
    with pytest.raises(ValueError, match="epochs=0"):
        ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="stream-ridge", epochs=0)
    with pytest.raises(ValueError, match="time_segments = 1"):
        ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="stream-ridge", time_segments=2)
    with pytest.raises(ValueError, match="needs epoch_plans"):
        ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="stream-ridge", epochs=2,
                           corrupt=(np.zeros((1, 16000), np.float32), None))
    with pytest.raises(ValueError, match="'stream-ridge'"):
        ex.main_from_audio(audio, labels, 32, "gammatone", "original", 0.6, readout="ridge")


def test_epoch_plans_draw_with_the_seed_plus_the_epoch():
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend
    augment = dict(noise_dir="synthetic", snr_db=(5.0, 20.0), time_shift_ms=100.0, level_db=0.0, seed=42)
    pace = dict(factors=[0.9, 1.0, 1.1], prob=1.0, seed=42)
    corrupt = cd.corruption(augment, 50)
    assert cd.epoch_plans(1, 50) == {}
    later = cd.epoch_plans(2, 50, augment, corrupt, None, None, pace)
    assert sorted(later) == ["mix", "speed"]
    again = cd.corruption(dict(augment, seed=44), 50)[1]
    for a, b in zip(later["mix"], again):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(later["speed"].choice, frontend.speed_plan(50, 3, prob=1.0, seed=44).choice)
    assert not np.array_equal(np.asarray(later["mix"].rows), np.asarray(corrupt[1].rows)) \
        or not np.array_equal(np.asarray(later["mix"].offsets), np.asarray(corrupt[1].offsets))
