"""SPEC.md 7 (include/lsm_hip_fit.h) restated in NumPy: the statistics of the streaming ridge fit after a block of rows, byte
for byte what the device leaves.  Row by row in ascending order, every accumulator continuing from its stored value."""
import numpy as np


def new_statistics(D, n_classes, upper=0.0):
    """The buffers as the caller initialises them; ``upper`` fills the strictly upper triangle of the Gram (a sentinel)."""
    gram = np.zeros((D, D), dtype=np.float64)
    gram[np.triu_indices(D, 1)] = upper
    return dict(gram=gram, class_sums=np.zeros((n_classes, D), dtype=np.float64),
                class_counts=np.zeros((n_classes,), dtype=np.int64), col_min=np.full((D,), np.inf, dtype=np.float32),
                col_max=np.full((D,), -np.inf, dtype=np.float32))


def accumulate(stats, features, labels, block=256):
    """``stats`` (a dict as `new_statistics` makes) after the rows ``features`` float32 (n, D) with ``labels`` int32 (n): new
    arrays, the strictly upper triangle of the Gram as it was."""
    x = np.asarray(features)
    assert x.dtype == np.float32 and x.ndim == 2
    labels = np.asarray(labels)
    assert labels.dtype == np.int32 and labels.shape == (x.shape[0],)
    out = {k: v.copy() for k, v in stats.items()}
    G, S, N, mn, mx = out["gram"], out["class_sums"], out["class_counts"], out["col_min"], out["col_max"]
    D, C = G.shape[0], S.shape[0]
    assert x.shape[1] == D
    with np.errstate(all="ignore"):
        for r in range(x.shape[0]):
            y = int(labels[r])
            if not 0 <= y < C:
                continue
            x64 = x[r].astype(np.float64)
            for lo in range(0, D, block):                  # G += np.outer(x64, x64), one block of rows at a time
                hi = min(lo + block, D)
                G[lo:hi, :hi] += x64[lo:hi, None] * x64[None, :hi]
            S[y] += x64
            N[y] += 1
            mn[:] = np.where(x[r] < mn, x[r], mn)
            mx[:] = np.where(x[r] > mx, x[r], mx)
    upper = np.triu_indices(D, 1)
    G[upper] = stats["gram"][upper]
    return out


def same_bytes(a, b):
    """Equal byte for byte, except that a NaN matches any NaN at the same position."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool((nan_a == nan_b).all()) and np.where(nan_a, 0, a).tobytes() == np.where(nan_b, 0, b).tobytes()


def lower(gram):
    """The lower triangle, packed row by row."""
    return gram[np.tril_indices(gram.shape[0])]
