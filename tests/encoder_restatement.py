"""What the spike encoder's range tests need beside the oracle (oracle/ref_numpy.py, oracle/cport.py): seeded dB
generators and the hysteresis latch of create_dataset.py:81-98 on explicit ON / OFF tables -- the C ABI takes tables, not
(thresholds, gap), so an OFF bound may lie above its ON bound or equal a value of the spectrogram.  TEST INFRASTRUCTURE ONLY;
held against tests/golden/encoder.npz by tests/test_encoder_host.py."""
from __future__ import annotations

import numpy as np


def overshoots(ncols: int, time_bins: int) -> bool:
    """Whether the last bin's resize coordinate (time_bins-1) * ((ncols-1)/(time_bins-1)) rounds to a double above
    ncols-1, i.e. lies outside the input, where scipy.ndimage.zoom answers cval = 0.0 (SPEC.md 1.2)."""
    if ncols == time_bins:
        return False
    zf = (ncols - 1) / (time_bins - 1)
    return (time_bins - 1) * zf > ncols - 1


# ---- dB generators ---------------------------------------------------------------------------------------------------

def walk_db(seed: int, n_clips: int, n_filters: int, ncols: int, dtype=np.float64) -> np.ndarray:
    """(n_clips, n_filters, ncols) random-walk dB rows around -30 dB, a few dozen dB wide: every threshold of a table in
    [0.1, 0.95] is crossed many times in both directions; the second half of the last clip runs backwards at half the
    swing (more crossings near the middle thresholds)."""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n_clips, n_filters, ncols)).cumsum(axis=2) * 4.0 - 30.0
    h = ncols // 2
    db[-1, :, h:] = db[-1, :, h:][:, ::-1] * 0.5
    return np.ascontiguousarray(db.astype(dtype))


def plateau_db(seed: int, n_clips: int, n_filters: int, ncols: int, dtype=np.float64) -> np.ndarray:
    """Rows that end HIGH: a random walk lifted by 30 dB over its last third (a ramp over the sixth before it), every third
    row a little more, so that latches are on in the last bins -- what the zero rule of an overshooting width must
    release."""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n_clips, n_filters, ncols)).cumsum(axis=2) * (12.0 / np.sqrt(ncols)) - 40.0
    t, r = max(2, ncols // 3), max(1, ncols // 6)
    db[:, :, ncols - t:] += 30.0
    db[:, :, ncols - t - r:ncols - t] += np.linspace(0.0, 30.0, r, endpoint=False)
    db[:, ::3, ncols - t:] += rng.uniform(2.0, 8.0, (n_clips, len(range(0, n_filters, 3)), 1))
    return np.ascontiguousarray(db.astype(dtype))


def step_rows(n_bins: int, dtype=np.float64) -> np.ndarray:
    """(rows, n_bins) normalised rows of two levels, 0.1 (below every OFF bound used) and 0.9 (above every ON bound used)
    plus one row at 0.5 between the bounds, with their edges at the first bin, the last bin and every 32-bin word
    boundary inside the row; two extra values fix the clip's range to [0, 1] (row 0 bin 1 = 0.0, row 1 bin 1 = 1.0 stay
    on their own side of the bounds).  Rows:
      0 never crosses (low everywhere)      1 on from bin 0 to the end (a latch held across every word)
      2 on in the first bin only            3 on in the last bin only
      then, for each word boundary w = 32, 64, ... < n_bins: on up to bin w-1 / on from bin w / on in bin w-1 only /
      on in bin w only / on at w-1, MIDDLE (0.5: holds the latch, sets none) from w on."""
    lo, hi, mid = 0.1, 0.9, 0.5
    rows = [np.full(n_bins, lo), np.full(n_bins, hi)]
    r = np.full(n_bins, lo); r[0] = hi; rows.append(r)
    r = np.full(n_bins, lo); r[-1] = hi; rows.append(r)
    for w in range(32, n_bins, 32):
        r = np.full(n_bins, lo); r[:w] = hi; rows.append(r)
        r = np.full(n_bins, lo); r[w:] = hi; rows.append(r)
        r = np.full(n_bins, lo); r[w - 1] = hi; rows.append(r)
        r = np.full(n_bins, lo); r[w] = hi; rows.append(r)
        r = np.full(n_bins, lo); r[w - 1] = hi; r[w:] = mid; rows.append(r)
    x = np.stack(rows)
    x[0, 1] = 0.0
    x[1, 1] = 1.0
    return np.ascontiguousarray(x.astype(dtype))


def db_of_norm(norm: np.ndarray) -> np.ndarray:
    """dB values in [-60, 0] whose min-max normalisation lands near `norm` (rows in [0, 1] holding a 0.0 and a 1.0); the
    tests take the EXACT normalised values from the oracle, this only places them."""
    return np.ascontiguousarray((norm.astype(np.float64) * 60.0 - 60.0).astype(norm.dtype))


# ---- the latch --------------------------------------------------------------------------------------------------------

def latch_loop(spec: np.ndarray, on, off) -> np.ndarray:
    """create_dataset.py:81-98, its loop as written, on tables: threshold k, ON bound on[k], OFF bound off[k] (both of the
    spectrogram's dtype, compared in it); rising and falling are taken from the latch before the update; output column
    time_bin * n_thr + k."""
    n_filters, n_time = spec.shape
    on = np.asarray(on, dtype=spec.dtype)
    off = np.asarray(off, dtype=spec.dtype)
    n_thr = len(on)
    spikes = np.zeros((n_filters, n_time * n_thr), dtype=np.uint8)
    for k in range(n_thr):
        active = np.zeros(n_filters, dtype=bool)
        for time_bin in range(n_time):
            rising = (spec[:, time_bin] > on[k]) & ~active
            falling = (spec[:, time_bin] < off[k]) & active
            active[rising] = True
            active[falling] = False
            spikes[:, time_bin * n_thr + k] = active.astype(np.uint8)
    return spikes


def latch_bits(spec: np.ndarray, on, off) -> np.ndarray:
    """The same latch with every (row, threshold) pair advanced together: active' = active ? !(x < off) : (x > on).  Equal
    to `latch_loop` (tests/test_encoder_host.py); used where a test encodes thousands of rows."""
    on = np.asarray(on, dtype=spec.dtype)
    off = np.asarray(off, dtype=spec.dtype)
    n_filters, n_time = spec.shape
    out = np.zeros((n_filters, n_time, len(on)), dtype=np.uint8)
    active = np.zeros((n_filters, len(on)), dtype=bool)
    with np.errstate(invalid="ignore"):
        for j in range(n_time):
            x = spec[:, j, None]
            active = np.where(active, ~(x < off[None, :]), x > on[None, :])
            out[:, j, :] = active
    return out.reshape(n_filters, n_time * len(on))


def tables(thresholds, gap: float, dtype):
    """ON thresholds sorted descending and the Python-float `thr - gap` OFF bounds, rounded to dtype
    (create_dataset.py:87-89)."""
    dt = np.dtype(dtype).type
    thr = sorted(thresholds, reverse=True)
    return np.array([dt(t) for t in thr], dtype=dt), np.array([dt(t - gap) for t in thr], dtype=dt)


def floored(db: np.ndarray) -> np.ndarray:
    """create_dataset.py:60 in the array's dtype: max(db, max(db) - 80); NaN propagates."""
    with np.errstate(invalid="ignore"):
        return np.maximum(db, db.max() - db.dtype.type(80.0))


def expected(oracle_c, db: np.ndarray, time_bins: int, on, off, apply_floor: bool = True, redundancy: int = 1):
    """One clip (n_filters, ncols) -> (normalised spectrogram (n_filters, time_bins), raster) as the reference computes
    them from these dB values: floor, C-oracle normalise + resize (SciPy-exact, tests/test_encoder_host.py), the latch
    above, row repeat."""
    with np.errstate(invalid="ignore"):
        norm = oracle_c.normalise_resize(floored(db) if apply_floor else db, time_bins)
    raster = latch_bits(norm, on, off) if len(on) else None
    if raster is not None and redundancy > 1:
        raster = np.repeat(raster, redundancy, axis=0)
    return norm, raster
