"""SPEC.md 1.9 restated in NumPy for the adaptive encoder's tests (test_adaptive_host.py, test_gpu_adaptive.py): column by
column, every operation in the dB array's own type and in the order the SPEC writes it -- the column extrema with > and <
(a NaN is skipped), the window over the last L columns, the floor before the minimum, the flat rule, the IEEE division."""
import numpy as np


def column_extrema(db):
    """(cmin, cmax) of every column of ``db`` (F, C): comparisons only, so a NaN never wins; a column with no other value
    keeps +inf / -inf."""
    T = db.dtype.type
    cmin = np.full(db.shape[1], np.inf, dtype=T)
    cmax = np.full(db.shape[1], -np.inf, dtype=T)
    for row in db:                                              # filter by filter, all columns at once
        cmax = np.where(row > cmax, row, cmax)
        cmin = np.where(row < cmin, row, cmin)
    return cmin, cmax


def _run(db, window_cols, cmin_before, cmax_before):
    """The columns of ``db`` behind the carried extrema of the columns before them (at most L - 1, oldest first)."""
    assert db.ndim == 2 and db.dtype in (np.float64, np.float32) and window_cols >= 1
    T, L = db.dtype.type, int(window_cols)
    F, C = db.shape
    k = len(cmin_before)
    assert k == len(cmax_before) <= L - 1
    cmin_new, cmax_new = column_extrema(db)
    cmin = np.concatenate([np.asarray(cmin_before, dtype=T), cmin_new])
    cmax = np.concatenate([np.asarray(cmax_before, dtype=T), cmax_new])
    norm = np.empty((F, C), dtype=T)
    lo_out, hi_out = np.empty(C, dtype=T), np.empty(C, dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            e = k + c
            first = max(0, e - L + 1)                           # columns before the stream's start do not exist
            hi, mn = T(-np.inf), T(np.inf)
            for i in range(first, e + 1):
                if cmax[i] > hi:
                    hi = cmax[i]
                if cmin[i] < mn:
                    mn = cmin[i]
            fl = T(hi - T(80.0))
            lo = mn if mn > fl else fl
            lo_out[c], hi_out[c] = lo, hi
            if T(hi - lo) < T(1e-8):                            # flat, or no value at all: -inf < 1e-8
                norm[:, c] = T(0)
                continue
            v = db[:, c]
            vf = np.where(v < fl, fl, v)                        # a NaN compares false and stays
            norm[:, c] = (vf - lo) / T(T(hi - lo) + T(1e-8))
    keep = min(L - 1, k + C)
    return norm, lo_out, hi_out, (cmin[len(cmin) - keep:], cmax[len(cmax) - keep:])


def adaptive(db, window_cols):
    """One stream from its start: ``db`` (F, C) float64 or float32 -> ``(norm (F, C), lo (C), hi (C))`` of the same type."""
    T = db.dtype.type
    norm, lo, hi, _ = _run(db, window_cols, np.zeros(0, dtype=T), np.zeros(0, dtype=T))
    return norm, lo, hi


def adaptive_cut(db, window_cols, cuts):
    """The same stream pushed in pieces of ``cuts`` columns: every push sees only the carried extrema and its own columns,
    as the kernel does.  Returns ``(norm, lo, hi, (cmin, cmax) carried at the end)``."""
    T = db.dtype.type
    carried = (np.zeros(0, dtype=T), np.zeros(0, dtype=T))
    parts, pos = [], 0
    for n in cuts:
        norm, lo, hi, carried = _run(db[:, pos:pos + n], window_cols, *carried)
        parts.append((norm, lo, hi))
        pos += n
    assert pos == db.shape[1]
    return (np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]), carried)
