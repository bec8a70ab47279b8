"""SPEC.md 1.13 restated in NumPy for the masked spike encoders' tests (test_mask_host.py, test_gpu_mask.py), on the oracle's
own steps (oracle/ref_numpy.py: normalise_resize, encode_hysteresis, pure_redundancy): the mask replaces values of the
normalised, resized spectrogram by +0.0 before the latches see them.  `plan_bits` restates `frontend.mask_plan`'s draws from
the text of SPEC.md 1.13.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import ref_numpy


def bits_of(words, n_bits: int) -> np.ndarray:
    """uint32 word rows (..., n_words) -> bool (..., n_bits): index i is bit i & 31 of word i >> 5; words and bits beyond
    n_bits are ignored."""
    words = np.asarray(words, dtype=np.uint32)
    i = np.arange(int(n_bits))
    return ((words[..., i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def words_of(bits) -> np.ndarray:
    """bool (n, n_bits) -> uint32 (n, ceil(n_bits / 32)), the layout `bits_of` reads."""
    bits = np.asarray(bits, dtype=bool)
    n, nb = bits.shape
    out = np.zeros((n, (nb + 31) // 32), dtype=np.uint32)
    for i in range(nb):
        out[:, i >> 5] |= bits[:, i].astype(np.uint32) << np.uint32(i & 31)
    return out


def masked_spectrogram(db, time_bins: int, apply_floor: bool, fm=None, tm=None) -> np.ndarray:
    """One clip's dB values (F, ncols) -> S' (F, time_bins): maximum, floor, minimum, the flat test and the resize are the
    unmasked clip's; then S'[f, j] = +0.0 where fm[f] or tm[j] (bool vectors or None)."""
    db = np.asarray(db)
    with np.errstate(invalid="ignore"):
        if apply_floor:
            db = np.maximum(db, db.max() - db.dtype.type(80.0))          # create_dataset.py:60
        S = np.array(ref_numpy.normalise_resize(db, int(time_bins)))
    F, Tb = S.shape
    cell = np.zeros((F, Tb), dtype=bool)
    if fm is not None:
        cell |= np.asarray(fm, dtype=bool)[:F, None]
    if tm is not None:
        cell |= np.asarray(tm, dtype=bool)[None, :Tb]
    S[cell] = 0.0
    return S


def masked_raster(db, time_bins: int, apply_floor: bool, thresholds, gap: float, redundancy: int, fm=None, tm=None):
    """One clip -> (S', raster (F * redundancy, time_bins * n_thr) uint8)."""
    S = masked_spectrogram(db, time_bins, apply_floor, fm, tm)
    with np.errstate(invalid="ignore"):
        raster = ref_numpy.pure_redundancy(ref_numpy.encode_hysteresis(S, thresholds, gap), int(redundancy))
    return S, raster


def masked_batch(db, time_bins: int, apply_floor: bool, thresholds, gap: float, redundancy: int, freq_words=None,
                 time_words=None):
    """(B, F, ncols) dB values and the ABI's word arrays (or None) -> (S' (B, F, time_bins), rasters)."""
    db = np.asarray(db)
    B, F, _ = db.shape
    fm = bits_of(freq_words, F) if freq_words is not None else [None] * B
    tm = bits_of(time_words, time_bins) if time_words is not None else [None] * B
    pairs = [masked_raster(db[b], time_bins, apply_floor, thresholds, gap, redundancy, fm[b], tm[b]) for b in range(B)]
    return np.stack([p[0].astype(db.dtype) for p in pairs]), np.stack([p[1] for p in pairs])


def zeroed_raster(raster, n_thr: int, redundancy: int, fm=None, tm=None) -> np.ndarray:
    """What masking is NOT: an unmasked raster (F * redundancy, time_bins * n_thr) with the masked rows and steps zeroed."""
    out = np.array(raster)
    if fm is not None:
        out[np.repeat(np.asarray(fm, dtype=bool), int(redundancy))] = 0
    if tm is not None:
        out[:, np.repeat(np.asarray(tm, dtype=bool), int(n_thr))] = 0
    return out


def plan_bits(n_clips: int, n_filters: int, time_bins: int, freq_masks=0, freq_width=0, time_masks=0, time_width=0,
              prob=1.0, seed=42):
    """SPEC.md 1.13's draws: generator RandomState([seed, 3]); (1) frequency widths randint(0, freq_width + 1, (n,
    freq_masks)); (2) frequency positions floor(random_sample * (F - width + 1)); (3), (4) the same pair for time;
    (5) u = random_sample(n), a clip with u >= prob has no mask.  Returns bool (n, F), bool (n, time_bins) and the bands
    ((positions, widths) for frequency and for time, before `prob`)."""
    rs = np.random.RandomState([seed, 3])
    n = n_clips
    fw = rs.randint(0, freq_width + 1, (n, freq_masks))
    fp = np.floor(rs.random_sample((n, freq_masks)) * (n_filters - fw + 1)).astype(int)
    tw = rs.randint(0, time_width + 1, (n, time_masks))
    tp = np.floor(rs.random_sample((n, time_masks)) * (time_bins - tw + 1)).astype(int)
    u = rs.random_sample(n)
    fm = np.zeros((n, n_filters), dtype=bool)
    tm = np.zeros((n, time_bins), dtype=bool)
    for c in range(n):
        if u[c] >= prob:
            continue
        for k in range(freq_masks):
            fm[c, fp[c, k]:fp[c, k] + fw[c, k]] = True
        for k in range(time_masks):
            tm[c, tp[c, k]:tp[c, k] + tw[c, k]] = True
    return fm, tm, ((fp, fw), (tp, tw))
