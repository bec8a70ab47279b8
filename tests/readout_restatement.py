"""SPEC.md §6 (readout scores) restated in NumPy: what ``lsm_readout_rows_f32`` and ``lsm_readout_windows`` must reproduce
byte for byte.  Imports nothing of the package: float64 array arithmetic in the pinned order only."""
import numpy as np

LANES = 64
MAX_CLASSES = 64


def scaled(features, mean, scale):
    """z = ((double)x - mean) / scale, (rows, D) float64: one subtraction, one true division."""
    x = np.asarray(features, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (x - np.asarray(mean, dtype=np.float64)) / np.asarray(scale, dtype=np.float64)


def logits_of(features, mean, scale, coef, intercept, n_keys, n_out):
    """(rows, C) float64: the 64 lane sums of every (row, class) in lane order, the tree, the intercept."""
    coef = np.asarray(coef, dtype=np.float64)
    intercept = np.asarray(intercept, dtype=np.float64)
    z = scaled(features, mean, scale)
    rows, D = z.shape
    C = coef.shape[0]
    assert D == n_keys * n_out and coef.shape == (C, D) and intercept.shape == (C,) and 1 <= C <= MAX_CLASSES
    p = np.zeros((rows, C, LANES), dtype=np.float64)
    with np.errstate(all="ignore"):
        for o0 in range(0, n_out, LANES):                   # the pass in which lane l takes neuron o0 + l
            live = min(LANES, n_out - o0)
            for k in range(n_keys):
                d = slice(k * n_out + o0, k * n_out + o0 + live)
                term = z[:, None, d] * coef[None, :, d]     # the product is rounded ...
                p[:, :, :live] = p[:, :, :live] + term      # ... then the sum
        s = LANES // 2
        while s >= 1:
            p[:, :, :s] = p[:, :, :s] + p[:, :, s:2 * s]
            s //= 2
        return intercept[None, :] + p[:, :, 0]


def labels_of(logits):
    """(rows) int32: -1 where a logit is NaN, else the first index of the largest logit."""
    logits = np.asarray(logits, dtype=np.float64)
    bad = np.isnan(logits).any(axis=1)
    best = np.where(bad[:, None], 0.0, logits).argmax(axis=1)           # argmax returns the first of equal maxima
    return np.where(bad, -1, best).astype(np.int32)


def scores(features, mean, scale, coef, intercept, n_keys, n_out):
    logits = logits_of(features, mean, scale, coef, intercept, n_keys, n_out)
    return logits, labels_of(logits)


def summation_bound(features, mean, scale, coef, intercept):
    """2 g (|b_c| + sum_d |z_d w_cd|), g = n u / (1 - n u), n = D + 2, u = 2^-53: how far two float64 evaluations of
    b_c + sum_d z_d w_cd in different summation orders can lie apart (each within g of the exact value of the rounded
    terms' sum; the intercept is one more term of the sum, hence D + 2 rather than D + 1 roundings)."""
    z = scaled(features, mean, scale)
    coef = np.asarray(coef, dtype=np.float64)
    n = z.shape[1] + 2
    u = 2.0 ** -53
    g = n * u / (1.0 - n * u)
    return 2.0 * g * (np.abs(np.asarray(intercept, dtype=np.float64))[None, :] + np.abs(z) @ np.abs(coef).T)


def debounce(labels, hold, background, state=None):
    """One stream's events [(window index, label)] for a label sequence, and the state to carry on: the event fires at the
    window in which the same label, neither background nor -1, has won ``hold`` consecutive windows; nothing more until the
    label changes."""
    last, run, seen = state if state is not None else (None, 0, 0)
    events = []
    for lab in labels:
        lab = int(lab)
        run = run + 1 if lab == last else 1
        last = lab
        if run == hold and lab != background and lab != -1:
            events.append((seen, lab))
        seen += 1
    return events, (last, run, seen)
