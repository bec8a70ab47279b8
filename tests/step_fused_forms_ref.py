"""CPU references and inputs shared by the tests of the masked and of the ragged one-launch step
(test_gpu_step_fused_masked.py, test_gpu_step_fused_ragged.py): the clips, thresholds and reservoir of
test_gpu_step_fused_range.py (two class chirps and one white-noise clip, thresholds (i + 1) / (n_thr + 1), k = N / 5), the
masks of each case, and what the C oracle and the NumPy restatement of SPEC.md 1.13 (tests/mask_restatement.py) give for a clip.
Nothing here touches a GPU: the conditions that keep the GPU comparisons from being vacuous can be checked with it alone.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402

_shapes, _reservoirs = {}, {}


def thresholds(n_thr):
    return [round((i + 1) / (n_thr + 1), 4) for i in range(n_thr)]


def clips(n_samples):
    from lsm_speech_classifier_amd import synth
    return np.ascontiguousarray(np.concatenate([synth.class_chirps([0, 5], seed=31, n_samples=n_samples),
                                                synth.white_noise(1, seed=9, n_samples=n_samples)]), dtype=np.float32)


class Shape:
    """The host side of `SpikeFrontEnd(F, "gammatone", thresholds=..., time_bins=bins, n_samples=bins * hop)`: strides, the
    coefficient table, thresholds and gap -- what the oracle's front end takes."""

    def __init__(self, F, bins, n_thr, hop, n_samples=None):
        from lsm_speech_classifier_amd import frontend
        self.F, self.bins, self.n_thr = F, bins, n_thr
        self.n_samples = bins * hop if n_samples is None else n_samples
        self.thresholds, self.gap = thresholds(n_thr), float(frontend.HYSTERESIS_GAP)
        hop_time = self.n_samples / (frontend.SAMPLE_RATE * bins)
        self.nwin, self.hop, self.ncols = frontend.gtgram_strides(frontend.SAMPLE_RATE, frontend.GT_WINDOW_TIME, hop_time,
                                                                  self.n_samples)
        self.tab = frontend.gammatone_filter_table(frontend.SAMPLE_RATE, F, frontend.GT_F_MIN)


def shape(F, bins, n_thr, hop, n_samples=None):
    key = (F, bins, n_thr, hop, n_samples)
    if key not in _shapes:
        _shapes[key] = Shape(*key)
    return _shapes[key]


def coef_table_3(tab):
    """The range test's second table: a channel-dependent A0, coef_flags 3 (no shared first-section gain)."""
    tab = np.array(tab)
    tab[:, 0] *= 1.0 + 1e-3 * np.arange(len(tab))
    return tab


def db_of(oracle_c, sh, clip, tab=None):
    with np.errstate(all="ignore"):
        return oracle_c.gammatone_db(oracle_c.gammatone_spec(clip, sh.tab if tab is None else tab, sh.nwin, sh.hop, sh.ncols))


def oracle_raster(oracle_c, sh, clip, tab=None):
    """The unmasked raster, all by the C oracle."""
    with np.errstate(all="ignore"):
        return oracle_c.encode_hysteresis(oracle_c.normalise_resize(db_of(oracle_c, sh, clip, tab), sh.bins), sh.thresholds,
                                          sh.gap)


def masked_raster(oracle_c, sh, clip, fm=None, tm=None, tab=None):
    """SPEC.md 1.13 restated (tests/mask_restatement.py) on the oracle's dB values: fm (F,), tm (bins,) bool or None."""
    with np.errstate(all="ignore"):
        return MR.masked_raster(db_of(oracle_c, sh, clip, tab), sh.bins, True, sh.thresholds, sh.gap, 1, fm, tm)[1]


def reservoir(oracle_c, F, bins, n_thr, hop, N):
    """The range test's reservoir of a shape: k = N / 5, 2 N / 5 output neurons, the critical weight of the oracle's rasters of
    the two chirps.  A host object (`snn.SNN(None, reservoir=...)` puts it on the GPU)."""
    key = (F, bins, n_thr, hop, N)
    if key not in _reservoirs:
        from lsm_speech_classifier_amd import reservoir as R
        from oracle import ref_numpy as O
        sh = shape(F, bins, n_thr, hop)
        audio = clips(sh.n_samples)
        rasters = np.stack([oracle_raster(oracle_c, sh, a) for a in audio[:2]])
        k = N // 5
        p = R.SimulationParams(num_neurons=N, num_output_neurons=2 * N // 5, small_world_graph_k=k,
                               mean_weight=O.w_critico(k, 2.0, 2, rasters) * 1.0)
        _reservoirs[key] = R.build_reservoir(p, F)
    return _reservoirs[key]


def lif(oracle_c, res, raster, keys=None):
    """(rows (n_keys * n_out,), stats [neurons that fired, spikes], spike matrix) of one clip by the C oracle."""
    feats, sm, _ = oracle_c.lif_run(res, raster, keys)
    return feats.reshape(-1), [int(sm.any(axis=0).sum()), int(sm.sum())], sm


def plan_of(fm, tm):
    """bool (B, F), bool (B, bins) -> frontend.MaskPlan."""
    from lsm_speech_classifier_amd import frontend
    return frontend.MaskPlan(MR.words_of(fm), MR.words_of(tm))


def form_masks(F=128, bins=16):
    """The masks of the six-form cases, one pair per clip: clip 0 two frequency bands (one across the 31|32 word edge) and
    time bins 5-7; clip 1 a frequency band and the first two and the last time bin; clip 2 (white noise) time bins 3-10 and
    filters 60-70."""
    fm, tm = np.zeros((3, F), dtype=bool), np.zeros((3, bins), dtype=bool)
    fm[0, 28:36] = fm[0, 100:104] = True
    tm[0, 5:8] = True
    fm[1, 10:20] = True
    tm[1, :2] = tm[1, bins - 1] = True
    fm[2, 60:71] = True
    tm[2, 3:11] = True
    return fm, tm


def edge_masks_97_33():
    """(97, 33, 1): filter 96 -- the only valid bit of the fourth frequency word -- and bin 32 -- the only valid bit of the
    second time word -- are masked on every clip, clip 1 also filters 40-59 and clip 2 bins 8-15; in the WORDS every bit at or
    beyond F and time_bins is set as well, and must be ignored."""
    fm, tm = np.zeros((3, 97), dtype=bool), np.zeros((3, 33), dtype=bool)
    fm[:, 96] = True
    tm[:, 32] = True
    fm[1, 40:60] = True
    tm[2, 8:16] = True
    plan = plan_of(fm, tm)
    freq, time = plan.freq.copy(), plan.time.copy()
    freq[:, 3] |= np.uint32(0xFFFFFFFE)
    time[:, 1] |= np.uint32(0xFFFFFFFE)
    return fm, tm, type(plan)(freq, time)


def straddle_masks(F=128, bins=100):
    """(128, 100, 4): four time words; bands across bins 31|32 (28-35) and 63|64 (60-67), clip 2 also bins 96-99 (the last
    word) and filters 0-15."""
    fm, tm = np.zeros((3, F), dtype=bool), np.zeros((3, bins), dtype=bool)
    tm[0, 28:36] = True
    tm[1, 60:68] = True
    fm[1, 64:80] = True
    tm[2, 28:36] = tm[2, 60:68] = tm[2, 96:100] = True
    fm[2, :16] = True
    return fm, tm


def resized_masks(F=128, bins=10):
    """(128, 10, 4) on hop 199: 8 columns resized to 10 bins, so the time mask indexes the resized bins: bins 2-3, bin 9 (the
    last, the zero-rule bin's place) and bins 0-4 with a frequency band."""
    fm, tm = np.zeros((3, F), dtype=bool), np.zeros((3, bins), dtype=bool)
    tm[0, 2:4] = True
    fm[0, 50:60] = True
    tm[1, 9] = True
    fm[1, 5:25] = True
    tm[2, :5] = True
    return fm, tm


def ragged_clip(oracle_c, F, n_thr, res, clip, t_b, tab3=False, keys=None):
    """A clip of `t_b` bins ALONE: the oracle's front end built for 160 * t_b samples and t_b bins, `lif_run` over its
    t_b * n_thr steps, features with T = t_b * n_thr.  Returns (rows, stats, raster)."""
    sh = shape(F, t_b, n_thr, 160)
    assert (sh.nwin, sh.hop, sh.ncols) == (400, 160, t_b - 2)
    raster = oracle_raster(oracle_c, sh, clip[:160 * t_b], coef_table_3(sh.tab) if tab3 else None)
    assert raster.shape == (F, t_b * n_thr)
    rows, stats, _ = lif(oracle_c, res, raster, keys)
    return rows, stats, raster
