"""Linear readouts on the device: StandardScaler, multinomial logistic regression
and a ridge classifier in PyTorch (ROCm on the GPU box, CPU tensors in the tests).

They mirror what the reference does on the host with scikit-learn
(/root/reference/extract_lsm_features.py:199-201 StandardScaler; /root/reference/train_classifier.py:36-45
LogisticRegression(multinomial, max_iter=1000)), plus the ridge readout that BASELINE.json configs[3]
names and the reference lacks.  BASELINE.json's north star keeps the readout in PyTorch on purpose: this
is plumbing around the hot path, not a hand-written kernel.  Parity target = scikit-learn on the same
arrays (tests/test_readout.py): identical predictions for ridge, >= 99 % agreement for logistic.
"""
from __future__ import annotations

from typing import NamedTuple

import torch


class StandardScaler:
    """sklearn.preprocessing.StandardScaler semantics: population variance, zero-variance columns
    are left unscaled, statistics in float64."""

    def fit(self, X: torch.Tensor):
        X64 = X.to(torch.float64)
        self.mean_ = X64.mean(dim=0)
        var = ((X64 - self.mean_) ** 2).mean(dim=0)
        self.scale_ = torch.where(var > 0, var.sqrt(), torch.ones_like(var))
        # sklearn treats variances at rounding-noise level as zero as well
        eps = torch.finfo(torch.float64).eps
        noise = var <= (X64.shape[0] * eps * var.new_tensor(1.0) * self.mean_.abs() ** 2 * 10)
        self.scale_ = torch.where(noise, torch.ones_like(var), self.scale_)
        return self

    def transform(self, X: torch.Tensor) -> torch.Tensor:
        return ((X.to(torch.float64) - self.mean_) / self.scale_).to(X.dtype if X.dtype.is_floating_point
                                                                     else torch.float64)

    def fit_transform(self, X: torch.Tensor) -> torch.Tensor:
        return self.fit(X).transform(X)


class RidgeReadout:
    """One-vs-rest ridge regression on {-1, +1} targets with an unpenalised intercept
    (sklearn.linear_model.RidgeClassifier): closed form in float64."""

    def __init__(self, alpha: float = 1.0):
        self.alpha = float(alpha)

    def fit(self, X: torch.Tensor, y: torch.Tensor):
        X64 = X.to(torch.float64)
        self.classes_ = torch.unique(y)
        Y = (y[:, None] == self.classes_[None, :]).to(torch.float64) * 2.0 - 1.0
        xm, ym = X64.mean(dim=0), Y.mean(dim=0)
        Xc, Yc = X64 - xm, Y - ym
        n, d = Xc.shape
        if d <= n:
            A = Xc.T @ Xc
            A.diagonal().add_(self.alpha)
            W = torch.linalg.solve(A, Xc.T @ Yc)
        else:                                            # dual form when features outnumber samples
            K = Xc @ Xc.T
            K.diagonal().add_(self.alpha)
            W = Xc.T @ torch.linalg.solve(K, Yc)
        self.coef_ = W.T.contiguous()
        self.intercept_ = ym - xm @ W
        return self

    def decision_function(self, X: torch.Tensor) -> torch.Tensor:
        return X.to(torch.float64) @ self.coef_.T + self.intercept_

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        return self.classes_[self.decision_function(X).argmax(dim=1)]


class LogisticReadout:
    """Multinomial logistic regression, L2 penalty 1/(2C) ||W||^2 on the coefficients (not on the
    intercept), full-batch L-BFGS in float64: the objective scikit-learn's lbfgs solver minimises."""

    def __init__(self, C: float = 1.0, max_iter: int = 1000, tol: float = 1e-6):
        self.C, self.max_iter, self.tol = float(C), int(max_iter), float(tol)

    def fit(self, X: torch.Tensor, y: torch.Tensor):
        X64 = X.to(torch.float64)
        self.classes_ = torch.unique(y)
        k, d = len(self.classes_), X64.shape[1]
        target = (y[:, None] == self.classes_[None, :]).to(torch.float64).argmax(dim=1)
        W = torch.zeros((k, d), dtype=torch.float64, device=X.device, requires_grad=True)
        b = torch.zeros(k, dtype=torch.float64, device=X.device, requires_grad=True)
        opt = torch.optim.LBFGS([W, b], lr=1.0, max_iter=self.max_iter, tolerance_grad=self.tol,
                                tolerance_change=1e-12, history_size=10, line_search_fn="strong_wolfe")

        def closure():
            opt.zero_grad()
            logits = X64 @ W.T + b
            loss = torch.nn.functional.cross_entropy(logits, target, reduction="sum") \
                + 0.5 / self.C * (W * W).sum()
            loss.backward()
            return loss

        opt.step(closure)
        self.coef_, self.intercept_ = W.detach(), b.detach()
        return self

    def decision_function(self, X: torch.Tensor) -> torch.Tensor:
        return X.to(torch.float64) @ self.coef_.T + self.intercept_

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        return self.classes_[self.decision_function(X).argmax(dim=1)]


# ---- a saved model and its scores on the device (SPEC.md §6, include/lsm_hip_readout.h) ----------------------------------
MAX_CLASSES = 64


def _f64(a) -> "np.ndarray":
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class LinearModel:
    """What turns a §4 feature row into a label: the scaler's ``mean`` / ``scale`` (D), the readout's ``coef`` (C, D) and
    ``intercept`` (C), all float64; ``classes`` (C) int64, the values ``class_of`` maps labels to, and optional
    ``class_names``; ``feature_keys`` and ``n_out`` with ``D = len(feature_keys) * n_out`` in §4's key-major order; and
    ``params``, a plain dict of the parameters the front end and the reservoir were built from (numbers, strings, flat lists).
    The refusals of SPEC.md §6 are made here: the device checks no model value."""

    def __init__(self, mean, scale, coef, intercept, classes, feature_keys, n_out: int, class_names=None, params=None):
        import numpy as np
        self.mean, self.scale, self.coef, self.intercept = _f64(mean), _f64(scale), _f64(coef), _f64(intercept)
        self.classes = np.ascontiguousarray(np.asarray(classes.cpu() if isinstance(classes, torch.Tensor) else classes,
                                                       dtype=np.int64))
        self.feature_keys = [str(k) for k in feature_keys]
        self.n_out = int(n_out)
        self.class_names = None if class_names is None else [str(n) for n in class_names]
        self.params = dict(params or {})
        D = len(self.feature_keys) * self.n_out
        C = self.coef.shape[0] if self.coef.ndim == 2 else -1
        if not 1 <= len(self.feature_keys) <= 8 or self.n_out < 1:
            raise ValueError(f"a model needs 1 to 8 feature keys and n_out >= 1, got {len(self.feature_keys)} and {self.n_out}")
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"coef must be (C, D) with 1 <= C <= {MAX_CLASSES}, got shape {self.coef.shape}")
        if (self.mean.shape != (D,) or self.scale.shape != (D,) or self.coef.shape != (C, D) or self.intercept.shape != (C,)
                or self.classes.shape != (C,) or (self.class_names is not None and len(self.class_names) != C)):
            raise ValueError(f"mismatched shapes: D = {len(self.feature_keys)} keys x {self.n_out} = {D}, C = {C}, but mean "
                             f"{self.mean.shape}, scale {self.scale.shape}, coef {self.coef.shape}, intercept "
                             f"{self.intercept.shape}, classes {self.classes.shape}")
        for name in ("mean", "scale", "coef", "intercept"):
            if not np.isfinite(getattr(self, name)).all():
                raise ValueError(f"{name} has a non-finite entry")
        if not (self.scale > 0).all():
            raise ValueError("scale must be > 0 everywhere")

    @property
    def n_classes(self) -> int:
        return int(self.coef.shape[0])

    @property
    def n_keys(self) -> int:
        return len(self.feature_keys)

    @classmethod
    def from_fitted(cls, scaler, clf, feature_keys, n_out: int, class_names=None, params=None):
        """From a fitted scaler and classifier: this module's ``StandardScaler`` / ``RidgeReadout`` / ``LogisticReadout`` or
        scikit-learn's objects (``mean_``, ``scale_``, ``coef_``, ``intercept_``, ``classes_``).  scikit-learn's single-row
        binary form becomes two rows -- row 0 all zeros with intercept 0, row 1 the fitted row --, so that the label is 1
        exactly where its ``decision_function`` is > 0 and a tie gives class 0."""
        import numpy as np
        coef, intercept = _f64(clf.coef_), _f64(clf.intercept_).reshape(-1)
        if coef.ndim == 1:
            coef = coef[None, :]
        classes = clf.classes_
        if coef.shape[0] == 1 and len(classes) == 2:
            coef = np.concatenate([np.zeros_like(coef), coef], axis=0)
            intercept = np.concatenate([np.zeros(1), intercept])
        return cls(scaler.mean_, scaler.scale_, coef, intercept, classes, feature_keys, n_out, class_names, params)

    def save(self, path) -> None:
        save_model_file(path, dict(mean=self.mean, scale=self.scale, coef=self.coef, intercept=self.intercept,
                                   classes=self.classes, class_names=self.class_names, feature_keys=self.feature_keys,
                                   n_out=self.n_out, params=self.params))

    @classmethod
    def load(cls, path):
        f = load_model_file(path)
        if "coef" not in f:
            raise ValueError(f"{path} holds the front half of a model only (scaler and parameters): no readout was saved")
        return cls(f["mean"], f["scale"], f["coef"], f["intercept"], f["classes"], f["feature_keys"], f["n_out"],
                   f.get("class_names"), f["params"])


def save_model_file(path, fields: dict) -> None:
    """An ``.npz`` of arrays and short strings only (nothing pickled): the arrays as they are, the string lists as unicode
    arrays, ``params`` as one JSON string."""
    import json
    import numpy as np
    out = {}
    for name in ("mean", "scale", "coef", "intercept"):
        if fields.get(name) is not None:
            out[name] = _f64(fields[name])
    if fields.get("classes") is not None:
        out["classes"] = np.asarray(fields["classes"], dtype=np.int64)
    if fields.get("class_names") is not None:
        out["class_names"] = np.array([str(n) for n in fields["class_names"]], dtype=np.str_)
    out["feature_keys"] = np.array([str(k) for k in fields["feature_keys"]], dtype=np.str_)
    out["n_out"] = np.int64(fields["n_out"])
    out["params_json"] = np.array(json.dumps(fields.get("params") or {}, sort_keys=True))
    with open(path, "wb") as fh:                 # a file object: np.savez appends no suffix to the caller's path
        np.savez(fh, **out)


def load_model_file(path) -> dict:
    """The fields ``save_model_file`` wrote, read with ``allow_pickle=False``."""
    import json
    import numpy as np
    with np.load(path, allow_pickle=False) as z:
        f = {name: z[name] for name in z.files}
    f["feature_keys"] = [str(k) for k in f["feature_keys"]]
    f["n_out"] = int(f["n_out"])
    f["params"] = json.loads(str(f.pop("params_json")))
    if "class_names" in f:
        f["class_names"] = [str(n) for n in f["class_names"]]
    return f


class DeviceReadout:
    """``model`` uploaded once to ``device``; scores on the device through ``lsm_readout_rows_f32`` and
    ``lsm_readout_windows``.  There is no host fallback."""

    def __init__(self, model: LinearModel, device=None):
        from . import _lib
        self._lib = _lib
        self.lib = _lib.load()
        _lib.require_gpu()
        self.model = model
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not self.lib.lsm_readout_supported(model.n_keys, model.n_out, model.n_classes):
            raise _lib.LsmHipError(f"no readout launch for {model.n_keys} keys x {model.n_out} output neurons, "
                                   f"{model.n_classes} classes")
        up = lambda a: torch.from_numpy(a).to(self.device).contiguous()     # noqa: E731
        self.mean, self.scale, self.coef, self.intercept = up(model.mean), up(model.scale), up(model.coef), up(model.intercept)
        self.classes = up(model.classes)

    def _model_args(self):
        from .frontend import _dev
        return [_dev(t) for t in (self.mean, self.scale, self.coef, self.intercept)]

    def score_rows(self, features):
        """``features`` float32 (..., D) on the device -> ``(logits, labels)``: float64 (..., C) and int32 (...)."""
        from .frontend import _dev
        m = self.model
        D = m.n_keys * m.n_out
        if features.dtype != torch.float32 or features.dim() < 1 or features.shape[-1] != D or features.device != self.device:
            raise ValueError(f"features must be float32 (..., {D}) on {self.device}, got {features.dtype} "
                             f"{tuple(features.shape)} on {features.device}")
        lead = tuple(features.shape[:-1])
        flat = features.reshape(-1, D).contiguous()
        n = int(flat.shape[0])
        logits = torch.zeros((n, m.n_classes), dtype=torch.float64, device=self.device)
        labels = torch.zeros((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._lib.check(self.lib.lsm_readout_rows_f32(
                *self._model_args(), _dev(flat), n, m.n_keys, m.n_out, m.n_classes, _dev(logits), _dev(labels), stream),
                "lsm_readout_rows_f32")
        return logits.reshape(lead + (m.n_classes,)), labels.reshape(lead)

    def score_windows(self, net, records, segment_steps: int, window_segments: int = 1, hop_segments: int = 1, segments=None):
        """``SNN.segment_features(records, ..., segments=...)`` followed by ``score_rows``, in one launch that writes no
        feature row: ``(logits, labels)``, float64 (B, W, C) and int32 (B, W).  Rows past a clip's windows are zeros and -1."""
        from .frontend import _dev, _host
        from .snn import _select_keys
        m = self.model
        if net.num_output_neurons != m.n_out or net.device != self.device:
            raise ValueError(f"the model was fitted on {m.n_out} output neurons, the reservoir has {net.num_output_neurons} "
                             f"(devices {self.device}, {net.device})")
        if (records.dtype != torch.int32 or records.dim() != 4 or tuple(records.shape[2:]) != (m.n_out, 4)
                or records.device != self.device):
            raise ValueError(f"records must be an int32 (B, G, {m.n_out}, 4) tensor on {self.device}")
        keys, key_ids = _select_keys(m.feature_keys)
        if keys != m.feature_keys:
            raise ValueError(f"the model's feature keys {m.feature_keys} are not all feature keys of the reservoir")
        records = records.contiguous()
        B, G = int(records.shape[0]), int(records.shape[1])
        W = net.segment_windows(G, window_segments, hop_segments)
        host_segments = net._host_segments(segments, B, G) if segments is not None else None
        logits = torch.zeros((B, W, m.n_classes), dtype=torch.float64, device=self.device)
        labels = torch.full((B, W), -1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            counts = net._device_counts(segments, host_segments) if segments is not None else None
            self._lib.check(self.lib.lsm_readout_windows(
                net._handle, *self._model_args(), _dev(records), B, G, _dev(counts), int(segment_steps), int(window_segments),
                int(hop_segments), _host(key_ids), len(keys), m.n_classes, _dev(logits), _dev(labels), stream),
                "lsm_readout_windows")
        return logits, labels

    def class_of(self, labels):
        """``classes[label]`` for labels >= 0 and -1 for -1: a tensor on the labels' device, or an array for an array."""
        import numpy as np
        if isinstance(labels, torch.Tensor):
            classes = self.classes.to(labels.device)
            return torch.where(labels >= 0, classes[labels.clamp(min=0).long()], torch.full_like(labels, -1, dtype=torch.int64))
        labels = np.asarray(labels)
        return np.where(labels >= 0, self.model.classes[np.clip(labels, 0, None)], -1)


# ---- training from statistics (SPEC.md §7, include/lsm_hip_fit.h) ----------------------------------------------------------
class RidgeSolution(NamedTuple):
    """What `RidgeStatistics.solve` returns, float64 on the statistics' device: the scaler's ``mean`` / ``scale`` (D), the
    readout's ``coef`` (C, D) and ``intercept`` (C) for the C classes that have rows, and those classes (int64)."""
    mean: torch.Tensor
    scale: torch.Tensor
    coef: torch.Tensor
    intercept: torch.Tensor
    classes: torch.Tensor


class RidgeStatistics:
    """What a `StandardScaler` and a `RidgeReadout` are functions of, in constant size: ``gram`` (D, D) float64, the lower
    triangle of X^T X (entries above the diagonal are never read); ``class_sums`` (C, D) float64; ``class_counts`` (C) int64;
    ``col_min`` / ``col_max`` (D) float32 -- all on one device.  `push` adds feature rows on the GPU (`lsm_fit_accumulate_f32`;
    there is no host fallback), `merge` adds another object's statistics, `save` / `load` keep them in a file, and `solve`
    gives the scaler and the readout that fitting on all pushed rows would give."""

    def __init__(self, feature_keys, n_out: int, n_classes: int, device=None):
        self.feature_keys = [str(k) for k in feature_keys]
        self.n_out, self.n_classes = int(n_out), int(n_classes)
        if not 1 <= len(self.feature_keys) <= 8 or self.n_out < 1 or not 1 <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"statistics need 1 to 8 feature keys, n_out >= 1 and 1 to {MAX_CLASSES} classes, got "
                             f"{len(self.feature_keys)}, {self.n_out} and {self.n_classes}")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        D, C = self.D, self.n_classes
        self.gram = torch.zeros((D, D), dtype=torch.float64, device=self.device)
        self.class_sums = torch.zeros((C, D), dtype=torch.float64, device=self.device)
        self.class_counts = torch.zeros((C,), dtype=torch.int64, device=self.device)
        self.col_min = torch.full((D,), float("inf"), dtype=torch.float32, device=self.device)
        self.col_max = torch.full((D,), float("-inf"), dtype=torch.float32, device=self.device)

    @property
    def D(self) -> int:
        return len(self.feature_keys) * self.n_out

    @property
    def rows(self) -> int:
        """How many rows the statistics hold (a host read of the counts)."""
        return int(self.class_counts.sum().item())

    def _fields(self):
        return self.gram, self.class_sums, self.class_counts, self.col_min, self.col_max

    @classmethod
    def from_arrays(cls, gram, class_sums, class_counts, col_min, col_max, feature_keys, n_out: int, device="cpu"):
        """From given statistics (arrays or tensors), on any device, the CPU included."""
        import numpy as np
        class_counts = np.asarray(class_counts.cpu() if isinstance(class_counts, torch.Tensor) else class_counts)
        self = cls(feature_keys, n_out, int(class_counts.shape[0]) if class_counts.ndim == 1 else -1, device)
        given = (_f64(gram), _f64(class_sums), np.ascontiguousarray(class_counts, dtype=np.int64),
                 np.ascontiguousarray(_np(col_min), dtype=np.float32), np.ascontiguousarray(_np(col_max), dtype=np.float32))
        for mine, theirs, name in zip(self._fields(), given, ("gram", "class_sums", "class_counts", "col_min", "col_max")):
            if tuple(mine.shape) != theirs.shape:
                raise ValueError(f"{name} must have shape {tuple(mine.shape)}, got {theirs.shape}")
            mine.copy_(torch.from_numpy(theirs))
        return self

    def push(self, features, labels) -> None:
        """Add the rows ``features`` float32 (n, D) with ``labels`` int32 (n), both on this object's GPU, on the current
        stream; a row whose label lies outside [0, n_classes) is skipped.  Pushes on one object must be stream-ordered by the
        caller."""
        from . import _lib
        from .frontend import _dev
        lib = _lib.load()
        _lib.require_gpu()
        if self.device.type != "cuda":
            raise _lib.LsmHipError(f"push runs on the GPU: these statistics live on {self.device} (there is no host fallback)")
        n = int(features.shape[0]) if features.dim() == 2 else -1
        if (features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] != self.D
                or features.device != self.device or not features.is_contiguous()):
            raise ValueError(f"features must be contiguous float32 (n, {self.D}) on {self.device}, got {features.dtype} "
                             f"{tuple(features.shape)} on {features.device}")
        if (labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or labels.device != self.device
                or not labels.is_contiguous()):
            raise ValueError(f"labels must be contiguous int32 ({n},) on {self.device}, got {labels.dtype} "
                             f"{tuple(labels.shape)} on {labels.device}")
        if not lib.lsm_fit_supported(len(self.feature_keys), self.n_out, self.n_classes):
            raise _lib.LsmHipError(f"no fit launch for {len(self.feature_keys)} keys x {self.n_out} output neurons, "
                                   f"{self.n_classes} classes")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(lib.lsm_fit_accumulate_f32(
                _dev(features), _dev(labels), n, len(self.feature_keys), self.n_out, self.n_classes,
                *[_dev(t) for t in self._fields()], stream), "lsm_fit_accumulate_f32")

    def merge(self, other: "RidgeStatistics") -> "RidgeStatistics":
        """Add ``other``'s statistics to these, in this order: gram, sums and counts by element-wise addition, then the
        minimum and the maximum of the ranges.  Defined to the bit, and in its last bits not what one run of pushes over both
        objects' rows leaves (SPEC.md §7)."""
        if (other.feature_keys, other.n_out, other.n_classes) != (self.feature_keys, self.n_out, self.n_classes):
            raise ValueError(f"statistics of {other.feature_keys} x {other.n_out}, {other.n_classes} classes do not merge into "
                             f"those of {self.feature_keys} x {self.n_out}, {self.n_classes} classes")
        theirs = [t.to(self.device) for t in other._fields()]
        self.gram += theirs[0]
        self.class_sums += theirs[1]
        self.class_counts += theirs[2]
        torch.minimum(self.col_min, theirs[3], out=self.col_min)
        torch.maximum(self.col_max, theirs[4], out=self.col_max)
        return self

    def packed_gram(self) -> "np.ndarray":
        """The lower triangle row by row, D * (D + 1) / 2 float64 values on the host."""
        import numpy as np
        g = self.gram.cpu().numpy()
        return np.concatenate([g[i, :i + 1] for i in range(self.D)])

    def save(self, path) -> None:
        """An ``.npz`` of arrays and short strings only (nothing pickled), the Gram as its packed lower triangle."""
        import numpy as np
        counts = self.class_counts.cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, gram_tril=self.packed_gram(), class_sums=self.class_sums.cpu().numpy(), class_counts=counts,
                     col_min=self.col_min.cpu().numpy(), col_max=self.col_max.cpu().numpy(),
                     feature_keys=np.array(self.feature_keys, dtype=np.str_), n_out=np.int64(self.n_out),
                     n_classes=np.int64(self.n_classes), rows=np.int64(counts.sum()))

    @classmethod
    def load(cls, path, device="cpu"):
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            f = {name: z[name] for name in z.files}
        keys, n_out, C = [str(k) for k in f["feature_keys"]], int(f["n_out"]), int(f["n_classes"])
        D = len(keys) * n_out
        if f["gram_tril"].shape != (D * (D + 1) // 2,) or f["class_counts"].shape != (C,) \
                or int(f["rows"]) != int(f["class_counts"].sum()):
            raise ValueError(f"{path}: not the statistics of {len(keys)} keys x {n_out}, {C} classes, {int(f['rows'])} rows")
        gram = np.zeros((D, D), dtype=np.float64)
        at = 0
        for i in range(D):
            gram[i, :i + 1] = f["gram_tril"][at:at + i + 1]
            at += i + 1
        return cls.from_arrays(gram, f["class_sums"], f["class_counts"], f["col_min"], f["col_max"], keys, n_out, device)

    def solve(self, alpha: float = 1.0) -> RidgeSolution:
        """`StandardScaler` + `RidgeReadout(alpha)` on the pushed rows, from the statistics alone (float64, on this object's
        device).  n = the counts' sum, mean = the class sums' sum / n.  A column whose range is one value is constant: its
        mean is that value, its scale 1, and it leaves the system (coefficient 0) -- exactly, where a variance from moments
        could only guess.  Otherwise var = max(G_ii / n - mean^2, 0) with the scaler's rounding-noise rule, and
        (diag(1/s) (G - n mean mean^T) diag(1/s) + alpha I) w_c = diag(1/s) (2 S_c - sum x - mean (2 n_c - n)), intercept
        (2 n_c - n) / n, one row per class that has rows."""
        counts = self.class_counts.to(torch.float64)
        n = counts.sum()
        if int(self.class_counts.sum().item()) == 0:
            raise ValueError("no rows have been pushed: nothing to solve")
        total = self.class_sums.sum(dim=0)
        lower = torch.tril(self.gram)
        G = lower + torch.tril(self.gram, -1).T
        constant = self.col_min == self.col_max
        mean = torch.where(constant, self.col_min.to(torch.float64), total / n)
        var = (G.diagonal() / n - mean * mean).clamp(min=0.0)
        eps = torch.finfo(torch.float64).eps
        noise = var <= n * eps * mean.abs() ** 2 * 10
        scale = torch.where((var > 0) & ~noise & ~constant, var.sqrt(), torch.ones_like(var))
        classes = torch.nonzero(self.class_counts > 0).reshape(-1)
        keep = torch.nonzero(~constant).reshape(-1)
        mk, sk = mean[keep], scale[keep]
        A = (G[keep][:, keep] - n * mk[:, None] * mk[None, :]) / sk[:, None] / sk[None, :]
        A.diagonal().add_(float(alpha))
        nc = counts[classes]
        rhs = (2.0 * self.class_sums[classes][:, keep] - total[keep] - mk[None, :] * (2.0 * nc - n)[:, None]) / sk[None, :]
        coef = torch.zeros((len(classes), self.D), dtype=torch.float64, device=self.device)
        if len(keep):
            coef[:, keep] = torch.linalg.solve(A, rhs.T).T
        return RidgeSolution(mean, scale, coef, (2.0 * nc - n) / n, classes)

    def to_model(self, alpha: float = 1.0, class_names=None, params=None) -> LinearModel:
        """The `LinearModel` of `solve(alpha)`; ``class_names``: one name per class of the statistics (all n_classes), of which
        the classes that have rows keep theirs."""
        s = self.solve(alpha)
        classes = s.classes.cpu().numpy()
        if class_names is not None:
            if len(class_names) != self.n_classes:
                raise ValueError(f"class_names must name all {self.n_classes} classes, got {len(class_names)}")
            class_names = [class_names[int(c)] for c in classes]
        return LinearModel(s.mean, s.scale, s.coef, s.intercept, classes, self.feature_keys, self.n_out, class_names, params)


def _np(a):
    import numpy as np
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
