"""SPEC.md 1.15 restated in NumPy for the silence trimmer's tests (test_trim_host.py, test_gpu_trim.py): the bin energies in
the pinned order, the activity test, the endpoint rule and the rows a launch writes, byte for byte."""
import numpy as np

HOP = 160
MIN_BINS = 3


def ratio_of(top_db):
    """What `frontend.SilenceTrimmer` passes: 10 ** (-top_db / 10), or 0.0 for top_db None (digital silence only)."""
    return 0.0 if top_db is None else 10.0 ** (-float(top_db) / 10.0)


def clip_length(count, n_samples):
    """len_b: any integer clamped to 0 .. n_samples; None (a NULL count array) is n_samples."""
    return int(n_samples) if count is None else int(min(max(int(count), 0), int(n_samples)))


def clip_bins(length, time_bins):
    return min(-(-int(length) // HOP), int(time_bins))


def energies(x, length, nb):
    """e_j for j < nb of one clip: float64, one accumulator per bin that starts at +0.0, i ascending (all bins advance
    together: the order WITHIN a bin is the pinned one).  Samples at or behind ``length`` are +0.0 and never read."""
    seg = np.zeros(nb * HOP, dtype=np.float64)
    have = min(int(length), nb * HOP)
    seg[:have] = np.asarray(x[:have], dtype=np.float32).astype(np.float64)
    seg = seg.reshape(nb, HOP)
    acc = np.zeros(nb, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(HOP):
            acc = acc + seg[:, i] * seg[:, i]
    return acc


def span(e, ratio, pad_bins, min_bins):
    """(first, bins) of a clip from its energies."""
    nb = len(e)
    if nb < MIN_BINS or not np.isfinite(e).all():
        return 0, nb
    level = np.float64(e.max()) * np.float64(ratio)
    active = np.nonzero(e > level)[0]
    if not len(active):
        return 0, nb
    lo = max(int(active[0]) - int(pad_bins), 0)
    hi = min(int(active[-1]) + int(pad_bins), nb - 1)
    m = min(int(min_bins), nb)
    if hi - lo + 1 < m:
        need = m - (hi - lo + 1)
        g = min(need, nb - 1 - hi)
        hi += g
        lo -= need - g
    return lo, hi - lo + 1


def trim(audio, clip_samples, time_bins, ratio, pad_bins, min_bins, n_samples_out=None):
    """What `lsm_trim_silence_f32` writes: ``audio`` (B, n_samples) float32, ``clip_samples`` B integers or None ->
    ``(audio_out (B, n_samples_out) float32, first (B,) int32, bins (B,) int32, energy (B, time_bins) float64)``."""
    audio = np.asarray(audio)
    assert audio.ndim == 2 and audio.dtype == np.float32
    B, n_samples = audio.shape
    n_out = HOP * int(time_bins) if n_samples_out is None else int(n_samples_out)
    assert n_out >= HOP * int(time_bins)
    out = np.zeros((B, n_out), dtype=np.float32)
    first, bins = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    energy = np.zeros((B, int(time_bins)), dtype=np.float64)
    for b in range(B):
        length = clip_length(None if clip_samples is None else clip_samples[b], n_samples)
        nb = clip_bins(length, time_bins)
        e = energies(audio[b], length, nb)
        energy[b, :nb] = e
        lo, n = span(e, ratio, pad_bins, min_bins)
        first[b], bins[b] = lo, n
        keep = min(max(length - HOP * lo, 0), HOP * n)
        out[b, :keep].view(np.uint32)[:] = audio[b, HOP * lo:HOP * lo + keep].view(np.uint32)
    return out, first, bins, energy


def slices(utterances, top_db=30.0, pad_bins=3, min_bins=3):
    """The host slices a trimmer names: every utterance (1-D float32, at least 3 bins) zero-padded to whole bins and cut to
    its span -> ``(list of 1-D float32 arrays of 160 * bins samples, first, bins)``."""
    cut, firsts, counts = [], [], []
    for u in utterances:
        u = np.asarray(u, dtype=np.float32)
        nb = -(-len(u) // HOP)
        row = np.zeros((1, nb * HOP), dtype=np.float32)
        row[0, :len(u)] = u
        out, first, bins, _ = trim(row, None, nb, ratio_of(top_db), pad_bins, min(max(min_bins, MIN_BINS), nb))
        cut.append(out[0, :HOP * int(bins[0])].copy())
        firsts.append(int(first[0]))
        counts.append(int(bins[0]))
    return cut, np.asarray(firsts, dtype=np.int32), np.asarray(counts, dtype=np.int32)
