"""Readout scores (SPEC.md 6, include/lsm_hip_readout.h), what can be checked without a GPU: the NumPy restatement
(tests/readout_restatement.py) against §6 written as loops and against decision_function within the bound the two summation
orders allow, the label rules, readout.LinearModel and its file, the header, binding and build lists, the launch functions'
refusals (made before any device work, so they run here) and pipeline.debounce."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_restatement as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_readout_supported", "lsm_readout_rows_f32", "lsm_readout_windows")
KEYS8 = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times', 'last_spike_times', 'mean_isi',
         'isi_variances', 'burst_counts']


def make_case(n_rows, n_keys, n_out, n_classes, seed):
    """Feature rows as the reservoir gives them (counts, times, exact zeros as after nan_to_num) and a model around them."""
    rng = np.random.default_rng(seed)
    D = n_keys * n_out
    x = (rng.integers(0, 40, (n_rows, D)) * rng.choice([0.0, 1.0, 0.37, 11.5], (n_rows, D))).astype(np.float32)
    x[rng.random((n_rows, D)) < 0.3] = 0.0
    mean = rng.standard_normal(D) * 3.0 + 5.0
    scale = rng.random(D) * 4.0 + 0.05
    coef = rng.standard_normal((n_classes, D)) * 0.1
    intercept = rng.standard_normal(n_classes)
    return x, mean, scale, coef, intercept


# ---- the restatement against the definition written as loops ---------------------------------------------------------------
def _loop_scores(x, mean, scale, coef, intercept, n_keys, n_out):
    """SPEC.md 6 for one row, one Python statement per sentence of the text."""
    C_ = coef.shape[0]
    logits = []
    for c in range(C_):
        p = [np.float64(0.0)] * 64
        for lane in range(64):
            for o in range(lane, n_out, 64):
                for k in range(n_keys):
                    d = k * n_out + o
                    z = (np.float64(x[d]) - mean[d]) / scale[d]
                    p[lane] = p[lane] + z * coef[c, d]
        for s in (32, 16, 8, 4, 2, 1):
            p = [p[lane] + p[lane + s] if lane < s else p[lane] for lane in range(64)]
        logits.append(intercept[c] + p[0])
    if any(np.isnan(v) for v in logits):
        return logits, -1
    label = 0
    for c in range(C_):
        if not any(logits[e] > logits[c] for e in range(C_)):
            label = c
            break
    return logits, label


@pytest.mark.parametrize("n_keys,n_out,n_classes", [(1, 1, 1), (5, 63, 2), (8, 64, 12), (1, 65, 64), (5, 130, 12), (8, 1, 2),
                                                     (1, 130, 1), (5, 64, 64), (8, 65, 2), (1, 63, 12)])
def test_the_restatement_equals_the_loops(n_keys, n_out, n_classes):
    x, mean, scale, coef, intercept = make_case(2, n_keys, n_out, n_classes, seed=n_out * 100 + n_keys * 10 + n_classes)
    logits, labels = RR.scores(x, mean, scale, coef, intercept, n_keys, n_out)
    assert logits.dtype == np.float64 and labels.dtype == np.int32 and logits.shape == (2, n_classes)
    with np.errstate(all="ignore"):
        for r in range(2):
            want, lab = _loop_scores(x[r], mean, scale, coef, intercept, n_keys, n_out)
            assert np.array(want, dtype=np.float64).tobytes() == logits[r].tobytes()
            assert int(labels[r]) == lab


def test_the_pinned_order_is_not_a_plain_dot_product():
    x, mean, scale, coef, intercept = make_case(16, 5, 130, 12, seed=4)
    logits, _ = RR.scores(x, mean, scale, coef, intercept, 5, 130)
    plain = RR.scaled(x, mean, scale) @ coef.T + intercept
    assert (logits != plain).any() and np.allclose(logits, plain, rtol=1e-9, atol=1e-9)


# ---- the restatement against decision_function ----------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:The number of unique classes")      # 64 classes on 96 samples, on purpose
@pytest.mark.parametrize("n_keys,n_out,n_classes", [(5, 130, 12), (8, 65, 2), (1, 63, 64)])
def test_the_restatement_lies_within_the_summation_bound_of_decision_function(n_keys, n_out, n_classes):
    import torch
    from sklearn.linear_model import RidgeClassifier
    from sklearn.preprocessing import StandardScaler as SkScaler
    from lsm_speech_classifier_amd import readout
    rng = np.random.default_rng(n_out)
    x, _, _, _, _ = make_case(96, n_keys, n_out, n_classes, seed=n_out)
    y = rng.integers(0, n_classes, 96)
    y[:n_classes] = np.arange(n_classes)
    # this package's objects
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    scaler = readout.StandardScaler().fit(xt)
    clf = readout.RidgeReadout(1.0).fit(scaler.transform(xt.to(torch.float64)), yt)
    model = readout.LinearModel.from_fitted(scaler, clf, KEYS8[:n_keys], n_out)
    got, labels = RR.scores(x, model.mean, model.scale, model.coef, model.intercept, n_keys, n_out)
    ref = clf.decision_function(scaler.transform(xt.to(torch.float64))).numpy()
    bound = RR.summation_bound(x, model.mean, model.scale, model.coef, model.intercept)
    assert got.shape == ref.shape == bound.shape and (np.abs(got - ref) <= bound).all()
    assert 0 < bound.max() < 1e-9
    # scikit-learn's
    sk_scaler = SkScaler().fit(x.astype(np.float64))
    sk = RidgeClassifier(alpha=1.0).fit(sk_scaler.transform(x.astype(np.float64)), y)
    sk_model = readout.LinearModel.from_fitted(sk_scaler, sk, KEYS8[:n_keys], n_out)
    got, labels = RR.scores(x, sk_model.mean, sk_model.scale, sk_model.coef, sk_model.intercept, n_keys, n_out)
    ref = sk.decision_function(sk_scaler.transform(x.astype(np.float64)))
    if ref.ndim == 1:                                                   # the binary form: one column, class 1's
        ref = np.stack([np.zeros_like(ref), ref], axis=1)
    bound = RR.summation_bound(x, sk_model.mean, sk_model.scale, sk_model.coef, sk_model.intercept)
    assert (np.abs(got - ref) <= bound).all()
    # the labels are the classifier's wherever its top-two margin exceeds what the orders can differ by
    top = np.sort(ref, axis=1)
    clear = (top[:, -1] - top[:, -2] > 2 * bound.max(axis=1)) if n_classes > 1 else np.ones(96, bool)
    assert clear.mean() > 0.9
    assert (sk_model.classes[labels[clear]] == sk.predict(sk_scaler.transform(x.astype(np.float64)))[clear]).all()


# ---- the label rules ------------------------------------------------------------------------------------------------------
def test_a_tie_gives_the_lower_index_and_a_nan_gives_minus_one_for_its_row_only():
    x, mean, scale, coef, intercept = make_case(3, 5, 65, 4, seed=9)
    coef[3], intercept[3] = coef[1], intercept[1]                       # two identical class rows
    big = np.abs(coef).max() * 50
    coef[1] = coef[3] = np.where(RR.scaled(x[:1], mean, scale)[0] >= 0, big, -big)      # and they win row 0
    logits, labels = RR.scores(x, mean, scale, coef, intercept, 5, 65)
    assert logits[0, 1] == logits[0, 3] == logits[0].max() and labels[0] == 1
    x[1, 77] = np.nan
    logits, labels2 = RR.scores(x, mean, scale, coef, intercept, 5, 65)
    assert labels2[1] == -1 and np.isnan(logits[1]).all() and labels2[0] == labels[0] and labels2[2] == labels[2]
    assert not np.isnan(logits[[0, 2]]).any()
    assert RR.labels_of(np.array([[-np.inf, -np.inf], [np.inf, np.inf], [1.0, np.inf]])).tolist() == [0, 0, 1]


# ---- LinearModel ----------------------------------------------------------------------------------------------------------
def _model(n_keys=5, n_out=7, n_classes=3, seed=1, **kw):
    from lsm_speech_classifier_amd import readout
    _, mean, scale, coef, intercept = make_case(1, n_keys, n_out, n_classes, seed)
    args = dict(mean=mean, scale=scale, coef=coef, intercept=intercept, classes=np.arange(n_classes) * 2 + 1,
                feature_keys=KEYS8[:n_keys], n_out=n_out, class_names=[f"w{c}" for c in range(n_classes)],
                params=dict(filterbank="gammatone", n_filters=32, seed=42, mean_weight=0.0123456789, thresholds=[0.1, 0.2]))
    args.update(kw)
    return readout.LinearModel(**args)


def test_linear_model_round_trip_returns_identical_bytes(tmp_path):
    from lsm_speech_classifier_amd import readout
    m = _model()
    path = str(tmp_path / "model.npz")
    m.save(path)
    assert os.path.exists(path)                                         # the caller's path, no suffix appended
    back = readout.LinearModel.load(path)
    for name in ("mean", "scale", "coef", "intercept", "classes"):
        a, b = getattr(m, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert back.feature_keys == m.feature_keys and back.n_out == 7 and back.class_names == ["w0", "w1", "w2"]
    assert back.params == m.params and back.n_classes == 3 and back.n_keys == 5
    with np.load(path, allow_pickle=False) as z:                        # arrays and short strings only
        assert all(z[k].dtype.kind in "fiU" for k in z.files)
    # the front half of a file is not a model
    readout.save_model_file(path, dict(mean=m.mean, scale=m.scale, feature_keys=m.feature_keys, n_out=7, params={}))
    with pytest.raises(ValueError, match="front half"):
        readout.LinearModel.load(path)


def test_linear_model_refusals(tmp_path):
    from lsm_speech_classifier_amd import readout
    good = _model()
    bad_scale = good.scale.copy()
    bad_scale[3] = 0.0
    with pytest.raises(ValueError, match="scale must be > 0"):
        _model(scale=bad_scale)
    bad_scale[3] = -1.0
    with pytest.raises(ValueError, match="scale must be > 0"):
        _model(scale=bad_scale)
    for name in ("mean", "scale", "coef", "intercept"):
        for v in (np.nan, np.inf):
            a = getattr(good, name).copy()
            a.flat[1] = v
            with pytest.raises(ValueError, match=f"{name} has a non-finite"):
                _model(**{name: a})
    with pytest.raises(ValueError, match="1 <= C <= 64"):
        _model(n_classes=65)
    _model(n_classes=64)
    with pytest.raises(ValueError, match="mismatched shapes"):
        _model(mean=good.mean[:-1])
    with pytest.raises(ValueError, match="mismatched shapes"):
        _model(intercept=good.intercept[:-1])
    with pytest.raises(ValueError, match="mismatched shapes"):
        _model(classes=np.arange(4))
    with pytest.raises(ValueError, match="mismatched shapes"):
        _model(feature_keys=KEYS8[:4])
    # load makes the same refusals
    path = str(tmp_path / "bad.npz")
    readout.save_model_file(path, dict(mean=good.mean, scale=bad_scale, coef=good.coef, intercept=good.intercept,
                                       classes=good.classes, feature_keys=good.feature_keys, n_out=7, params={}))
    with pytest.raises(ValueError, match="scale must be > 0"):
        readout.LinearModel.load(path)


def test_the_binary_scikit_learn_form_predicts_as_scikit_learn_does():
    from sklearn.linear_model import LogisticRegression, RidgeClassifier
    from sklearn.preprocessing import StandardScaler as SkScaler
    from lsm_speech_classifier_amd import readout
    rng = np.random.default_rng(5)
    x = rng.standard_normal((80, 10)).astype(np.float32)
    y = np.where(x[:, 0] + 0.5 * x[:, 3] + 0.3 * rng.standard_normal(80) > 0, 7, 3)
    scaler = SkScaler().fit(x.astype(np.float64))
    for clf in (RidgeClassifier(alpha=1.0), LogisticRegression(max_iter=1000)):
        clf.fit(scaler.transform(x.astype(np.float64)), y)
        assert np.atleast_2d(clf.coef_).shape == (1, 10)                # one row for two classes
        m = readout.LinearModel.from_fitted(scaler, clf, KEYS8[:2], 5)
        assert m.coef.shape == (2, 10) and not m.coef[0].any() and m.intercept[0] == 0.0 and m.classes.tolist() == [3, 7]
        logits, labels = RR.scores(x, m.mean, m.scale, m.coef, m.intercept, 2, 5)
        assert (m.classes[labels] == clf.predict(scaler.transform(x.astype(np.float64)))).all()
        assert 10 < (labels == 1).sum() < 70
    # a tie (decision 0) gives class 0, as `decision > 0` does
    m0 = readout.LinearModel(np.zeros(2), np.ones(2), np.array([[0.0, 0.0], [1.0, -1.0]]), np.zeros(2), [3, 7], KEYS8[:2], 1)
    assert RR.scores(np.array([[2.0, 2.0]], np.float32), m0.mean, m0.scale, m0.coef, m0.intercept, 2, 1)[1].tolist() == [0]


# ---- header, binding, build -------------------------------------------------------------------------------------------------
def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_binding_and_library_carry_the_three_names(tmp_path):
    import shutil
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_readout.h")).read()
    assert _params(header, "lsm_readout_supported") == ["int n_keys", "int n_out", "int n_classes"]
    assert _params(header, "lsm_readout_rows_f32") == [
        "const double *mean", "const double *scale", "const double *coef", "const double *intercept", "const float *features",
        "int n_rows", "int n_keys", "int n_out", "int n_classes", "double *logits_out", "int32_t *labels_out", "void *stream"]
    assert _params(header, "lsm_readout_windows") == [
        "const lsm_reservoir *h", "const double *mean", "const double *scale", "const double *coef", "const double *intercept",
        "const void *records", "int n_clips", "int n_segments", "const int32_t *clip_segments", "int segment_steps",
        "int window_segments", "int hop_segments", "const int32_t *key_ids", "int n_keys", "int n_classes",
        "double *logits_out", "int32_t *labels_out", "void *stream"]
    assert _lib.READOUT_SYMBOLS == tuple(_lib.READOUT_SIGS) == NEW
    for name in NEW:
        res, args = _lib.READOUT_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params)
        for p, ctype in zip(params, args):
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    older = [_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
             _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS, _lib.RAGGED_SIGS, _lib.STEP_SIGS,
             _lib.STEP_STATE_SIGS, _lib.TRIM_SIGS, _lib.RAGGED_AUGMENT_SIGS]
    assert sum(len(t) for t in older) == 83 and len(set().union(*older)) == 83      # the fifteen older tables keep their sizes
    assert not set(NEW) & set().union(*older)
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert "readout.hip" in build.SOURCES and "lsm_hip_readout.h" in build.ABI_HEADERS
    assert "reservoir_facts.h" in build.HEADERS and len(build.PUBLIC_HEADERS) == 9
    # the header is hashed into the build id: another text of it, another id
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(include_dir=str(inc)) == build.source_id()
    with open(inc / "lsm_hip_readout.h", "a") as f:
        f.write("/* changed */\n")
    assert build.source_id(include_dir=str(inc)) != build.source_id()


def test_supported_sizes():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    assert lib.lsm_readout_supported(1, 1, 1) == 1 and lib.lsm_readout_supported(8, 8192, 64) == 1
    for bad in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 8193, 1), (1, 1, 0), (1, 1, 65)):
        assert lib.lsm_readout_supported(*bad) == 0


M, S_, W_, B_, X, L, O, R, CS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000


def _in_order(call, later, texts):
    """Each row breaks its own rule AND every later one: the message names the earliest."""
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)


def test_rows_refusals_in_their_order():
    """Every refusal is made on the host before anything is launched, so fake (aligned, distinct) addresses serve."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    good = dict(mean=M, scale=S_, coef=W_, intercept=B_, features=X, n_rows=3, n_keys=5, n_out=70, n_classes=12, logits=O,
                labels=L)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_readout_rows_f32(a["mean"] or None, a["scale"] or None, a["coef"] or None, a["intercept"] or None,
                                      a["features"] or None, a["n_rows"], a["n_keys"], a["n_out"], a["n_classes"],
                                      a["logits"] or None, a["labels"] or None, None)
        return rc, lib.lsm_last_error().decode()

    later = [dict(n_rows=-1), dict(n_keys=9), dict(n_out=0), dict(n_classes=65), dict(coef=0), dict(logits=0, labels=0),
             dict(mean=M + 4), dict(labels=L + 2)]
    texts = ["n_rows=-1", "n_keys=9", "n_out=0", "n_classes=65", "are required", "both NULL", "8-byte aligned", "4-byte aligned"]
    # the row that breaks "both NULL" cannot also carry a misaligned labels: those two are checked one by one below
    _in_order(call, later[:6], texts[:6])
    _in_order(call, later[6:], texts[6:])
    for kw, text in ((dict(n_keys=0), "n_keys=0"), (dict(n_out=8193), "n_out=8193"), (dict(n_classes=0), "n_classes=0"),
                     (dict(mean=0), "are required"), (dict(scale=0), "are required"), (dict(intercept=0), "are required"),
                     (dict(scale=S_ + 1), "8-byte aligned"), (dict(coef=W_ + 4), "8-byte aligned"),
                     (dict(intercept=B_ + 2), "8-byte aligned"), (dict(logits=O + 4), "8-byte aligned"),
                     (dict(features=X + 2), "4-byte aligned"), (dict(features=0), "null features")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert call(n_rows=0)[0] == 0 and call(n_rows=0, features=0)[0] == 0          # nothing to do, nothing launched


def test_windows_refusals_in_their_order():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    H = 0xABC000                                                        # a handle is not read before the last refusal
    keys = (C.c_int32 * 8)(0, 1, 2, 5, 6, 0, 0, 0)
    bad_keys = (C.c_int32 * 8)(0, 1, 8, 5, 6, 0, 0, 0)
    good = dict(h=H, mean=M, scale=S_, coef=W_, intercept=B_, records=R, n_clips=2, n_segments=6, clip_segments=CS,
                segment_steps=8, window=3, hop=1, keys=keys, n_keys=5, n_classes=12, logits=O, labels=L)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_readout_windows(a["h"] or None, a["mean"] or None, a["scale"] or None, a["coef"] or None,
                                     a["intercept"] or None, a["records"] or None, a["n_clips"], a["n_segments"],
                                     a["clip_segments"] or None, a["segment_steps"], a["window"], a["hop"],
                                     C.cast(a["keys"], C.c_void_p) if a["keys"] is not None else None, a["n_keys"],
                                     a["n_classes"], a["logits"] or None, a["labels"] or None, None)
        return rc, lib.lsm_last_error().decode()

    later = [dict(h=0), dict(n_segments=0), dict(segment_steps=0), dict(window=7), dict(hop=0), dict(n_keys=9),
             dict(n_classes=0), dict(mean=0), dict(logits=0, labels=0), dict(records=R + 8), dict(coef=W_ + 4),
             dict(clip_segments=CS + 2)]
    texts = ["null handle", "bad n_clips/n_segments", "segment_steps=0", "window_segments=7", "hop_segments=0",
             "n_keys must be", "n_classes=0", "are required", "both NULL", "16-byte aligned", "8-byte aligned", "4-byte aligned"]
    _in_order(call, later, texts)
    for kw, text in ((dict(n_clips=-1), "bad n_clips"), (dict(window=0), "window_segments=0"),
                     (dict(segment_steps=30000, window=3), "exceeds 65535"), (dict(keys=None), "n_keys must be"),
                     (dict(keys=bad_keys), "key id 8"), (dict(n_classes=65), "n_classes=65"),
                     (dict(intercept=0), "are required"), (dict(logits=O + 4), "8-byte aligned"),
                     (dict(labels=L + 1), "4-byte aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    # the window limit comes before the keys, the keys before the classes
    assert "exceeds 65535" in call(segment_steps=30000, n_keys=9)[1] and "key id 8" in call(keys=bad_keys, n_classes=0)[1]
    assert call(n_clips=0)[0] == 0 and call(n_clips=0, records=0)[0] == 0         # nothing to do, nothing launched
    rc, msg = call(records=0, logits=0)
    assert rc == -1 and "null records" in msg


def test_push_scores_without_a_readout_raises():
    from lsm_speech_classifier_amd import pipeline
    bank = pipeline.StreamBank.__new__(pipeline.StreamBank)
    bank.readout = None
    with pytest.raises(ValueError, match="needs a readout"):
        bank.push_scores(None, None)
    audio_bank = pipeline.AudioStreamBank.__new__(pipeline.AudioStreamBank)
    audio_bank.bank = bank
    with pytest.raises(ValueError, match="needs a readout"):
        audio_bank.push_scores(None)


# ---- debounce ---------------------------------------------------------------------------------------------------------------
def _events_in_pushes(seqs, cuts, hold, background):
    """The events of the label sequences ``seqs`` delivered in pushes that end at ``cuts[b]`` (ascending positions)."""
    from lsm_speech_classifier_amd import pipeline
    n = len(seqs)
    n_push = max(len(c) for c in cuts) + 1
    state, events = None, []
    at = [0] * n
    for push in range(n_push):
        ends = [c[push] if push < len(c) else len(seqs[b]) for b, c in enumerate(cuts)]
        counts = np.array([ends[b] - at[b] for b in range(n)])
        labels = np.full((n, max(int(counts.max()), 1)), 99, dtype=np.int32)        # what lies past a count is never read
        for b in range(n):
            labels[b, :counts[b]] = seqs[b][at[b]:ends[b]]
        ev, state = pipeline.debounce(labels, counts, state, hold, background)
        events += ev
        at = ends
    return sorted(events)


def test_debounce_gives_the_same_events_however_the_sequence_is_cut():
    rng = np.random.default_rng(2)
    seqs = [np.repeat(rng.integers(-1, 4, 14), rng.integers(1, 5, 14)).tolist() for _ in range(3)]
    for hold in (1, 2, 3):
        whole = _events_in_pushes(seqs, [[], [], []], hold, background=0)
        want = sorted((b, w, lab) for b in range(3) for w, lab in RR.debounce(seqs[b], hold, 0)[0])
        assert whole == want and len(whole) >= 3
        assert all(lab not in (0, -1) for _, _, lab in whole)                       # background and -1 never fire
        for cut in range(0, len(seqs[0]) + 1):                                      # stream 0 cut anywhere, the others elsewhere
            assert _events_in_pushes(seqs, [[cut], [3, 5], []], hold, 0) == whole
        assert _events_in_pushes(seqs, [list(range(1, len(s))) for s in seqs], hold, 0) == whole    # one label per push


def test_debounce_hold_and_change_rules():
    from lsm_speech_classifier_amd import pipeline

    def run(seq, hold, background=0):
        return [(w, lab) for _, w, lab in pipeline.debounce(np.array([seq]), np.array([len(seq)]), None, hold, background)[0]]

    assert run([2, 2, 2, 2, 0, 2, 2, 3, 3, 3], 2) == [(1, 2), (6, 2), (8, 3)]
    assert run([2, 2, 2, 2, 0, 2, 2, 3, 3, 3], 1) == [(0, 2), (5, 2), (7, 3)]       # hold = 1: at the first window
    assert run([2, 2, 2, 2, 0, 2, 2, 3, 3, 3], 3) == [(2, 2), (9, 3)]
    assert run([0, 0, 0, -1, -1, -1], 2) == [] and run([5, 5, 5], 2, background=5) == []
    assert run([0, 0, 0], 1, background=7) == [(0, 0)]                              # label 0 is a label like any other
    with pytest.raises(ValueError, match="hold"):
        pipeline.debounce(np.zeros((1, 1), np.int32), np.array([1]), None, 0, 0)
    # a stream that receives nothing keeps its state
    ev, st = pipeline.debounce(np.array([[4, 4], [4, 9]]), np.array([1, 0]), None, 2, 0)
    ev2, _ = pipeline.debounce(np.array([[4, 4], [4, 9]]), np.array([1, 2]), st, 2, 0)
    assert ev == [] and ev2 == [(0, 1, 4)]
