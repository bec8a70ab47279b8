"""SPEC.md 1.16 restated for the tests of the ragged mixer and of the masks on ragged launches (test_ragged_augment_host.py,
test_gpu_ragged_mix.py, test_gpu_ragged_masks.py, test_gpu_step_fused_ragged_masked.py, test_gpu_ragged_augment_pipeline.py).
The definition is "the clip alone", so each restatement is a loop over the clips that calls the existing restatement
(tests/mix_restatement.py, tests/mask_restatement.py over the oracle) at the clip's own shape, and then lays the result into
the launch's strides.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402
import mix_restatement as MX  # noqa: E402

HOP = 160


def clamp_samples(clip_samples, n_samples: int) -> np.ndarray:
    return np.clip(np.asarray(clip_samples, dtype=np.int64), 0, int(n_samples))


def mix_ragged(audio, clip_samples, noise, ratio, rows, offsets, shift, scale):
    """The ragged batch form -> ``(y float32 (B, n_samples), g float64 (B), powers float64 (B, 2))``: clip b is
    `mix_restatement.mix` on ``audio[b, :n_b]`` alone; the row is +0.0 from n_b on; n_b = 0 gives g = 0 and powers +0.0."""
    audio = np.asarray(audio)
    B, n = audio.shape
    nb = clamp_samples(clip_samples, n)
    y = np.zeros((B, n), dtype=np.float32)
    g = np.zeros(B, dtype=np.float64)
    powers = np.zeros((B, 2), dtype=np.float64)
    for b in range(B):
        if nb[b] == 0:
            continue
        yb, gb, pb = MX.mix(audio[b:b + 1, :nb[b]], noise, np.asarray(ratio)[b:b + 1], np.asarray(rows)[b:b + 1],
                            np.asarray(offsets)[b:b + 1], np.asarray(shift)[b:b + 1], np.asarray(scale)[b:b + 1])
        y[b, :nb[b]], g[b], powers[b] = yb[0], gb[0], pb[0]
    return y, g, powers


def clamp_bins(bins, time_bins: int) -> np.ndarray:
    """SPEC.md 1.14's clamp: 0, or 3 .. time_bins."""
    t = np.clip(np.asarray(bins, dtype=np.int64), 0, int(time_bins))
    return np.where(t < 3, 0, t)


def masked_ragged(dbs, bins, time_bins: int, apply_floor: bool, thresholds, gap: float, redundancy: int, freq_words=None,
                  time_words=None, dtype=np.float64):
    """``dbs[b]``: clip b's own dB values (F, cols_b) (ignored for a clip of 0 bins); ``bins[b]`` its T_b; the words at the
    launch's strides.  -> ``(S' (B, F, time_bins), rasters (B, F * redundancy, time_bins * n_thr))`` with clip b's
    `mask_restatement.masked_raster` at (cols_b, T_b) under the first F and T_b bits of its rows, zeros behind."""
    B = len(bins)
    F = next(np.asarray(d).shape[0] for d, t in zip(dbs, bins) if t)
    n_thr = len(thresholds)
    S = np.zeros((B, F, time_bins), dtype=dtype)
    raster = np.zeros((B, F * redundancy, time_bins * n_thr), dtype=np.uint8)
    for b, T in enumerate(clamp_bins(bins, time_bins)):
        if T == 0:
            continue
        fm = MR.bits_of(freq_words[b], F) if freq_words is not None else None
        tm = MR.bits_of(time_words[b], T) if time_words is not None else None
        s, r = MR.masked_raster(np.asarray(dbs[b], dtype=dtype), int(T), apply_floor, thresholds, gap, redundancy, fm, tm)
        S[b, :, :T], raster[b, :, :T * n_thr] = s, r
    return S, raster


def gammatone_db(oracle_c, tab, clip, t_b: int):
    """The oracle's dB values (F, t_b - 2) of a clip of ``t_b`` bins alone: gtgram with (400, 160, t_b - 2) on its first
    160 * t_b samples."""
    with np.errstate(all="ignore"):
        return oracle_c.gammatone_db(oracle_c.gammatone_spec(np.ascontiguousarray(clip[:HOP * t_b]), tab, 400, HOP, t_b - 2))


def ragged_time_bands(bins, time_bins: int, time_masks: int, time_width: int, freq_masks: int, freq_width: int, n_filters: int,
                      prob: float, seed: int):
    """`frontend.mask_plan_ragged`'s draws restated from SPEC.md 1.16: `mask_restatement.plan_bits`' five steps in their order,
    the time bands with w_eff = min(w, T_b) at floor(u * (T_b - w_eff + 1)).  -> (bool (n, F), bool (n, time_bins), the time
    bands (positions, effective widths) before `prob`)."""
    rs = np.random.RandomState([seed, 3])
    n = len(bins)
    bins = np.asarray(bins, dtype=np.int64)
    fw = rs.randint(0, freq_width + 1, (n, freq_masks))
    fp = np.floor(rs.random_sample((n, freq_masks)) * (n_filters - fw + 1)).astype(int)
    tw = np.minimum(rs.randint(0, time_width + 1, (n, time_masks)), bins[:, None])
    tp = np.floor(rs.random_sample((n, time_masks)) * (bins[:, None] - tw + 1)).astype(int)
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
    return fm, tm, (tp, tw)
