"""SPEC.md 1.5 restated in NumPy for the per-bin mel tests (test_mel_bins_host.py, test_gpu_mel_bins.py): the float64 power
spectrum of a frame by a direct DFT (no FFT library), the centred frames, the kernels' mel projection in float32 operation
for operation (four interleaved partial sums, every product rounded and then added: the build has `-ffp-contract=off`), the
per-bin tolerance, and the seeded clips and bases both tests use, so that the host test vouches for the bytes the GPU test
sends."""
import numpy as np

N_FFT = 2048
N_BINS = N_FFT // 2 + 1
SHAPES = [(4096, 1024), (1500, 333), (333, 33)]            # (n_samples, hop)
IMPULSE_POSITIONS = (1, 2, 17, 1023, 1024, 1025, 2046, 2047)
IMPULSE_LEVEL = np.float32(0.75)
TONE_BINS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1022, 1023, 1024)
NOISE_SCALES = (0.1, 1e-4, 1e3)
MAX_WIDTH = 72
FILL = np.float32(1e30)                                     # the basis outside [lo, hi): a read out of range shows
TINY = float(np.finfo(np.float32).tiny)
_CACHE = {}


def hann_periodic(n=N_FFT):
    """scipy.signal.get_window('hann', n, fftbins=True), float64 (oracle/ref_numpy.py and mel.stft_tables: the same bits)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _dft_matrices():
    """cos and sin of 2 pi k n / 2048, (1025, 2048) float64, the angle from (k n) mod 2048: the reduction is exact."""
    if "dft" not in _CACHE:
        k, n = np.arange(N_BINS, dtype=np.int64)[:, None], np.arange(N_FFT, dtype=np.int64)[None, :]
        angle = ((k * n) % N_FFT).astype(np.float64) * (2.0 * np.pi / N_FFT)
        _CACHE["dft"] = (np.cos(angle), np.sin(angle))
    return _CACHE["dft"]


def windowed(frames):
    """hann_periodic(2048) * frame in float64: (..., 2048) float32 -> (..., 2048) float64."""
    frames = np.asarray(frames)
    assert frames.dtype == np.float32 and frames.shape[-1] == N_FFT
    return hann_periodic() * frames.astype(np.float64)


def dft_power64(frames):
    """float64 |X[k]|^2, k = 0..1024, of the windowed frames: (..., 2048) float32 -> (..., 1025) float64."""
    cos, sin = _dft_matrices()
    wx = windowed(frames)
    re, im = wx @ cos.T, wx @ sin.T
    return re * re + im * im


def transform_error(frames):
    """e = 64 * 2^-53 * sum_n |w[n] x[n]| per frame: the bound on the float64 transform's own error in |X[k]|."""
    return 64.0 * 2.0 ** -53 * np.abs(windowed(frames)).sum(axis=-1)


def bin_tolerance(p_ref, e, h):
    """The bound on |P - P_ref| of a bin: re and im rounded to float32 (2^-24 of |X| each), hypotf within h ulps (h 2^-23),
    one rounding for the square (2^-24): (1.5 + 2 h) 2^-23 P_ref; and a transform off by e in |X|: 2 sqrt(P_ref) e + e^2.
    ``e``: one value per frame, broadcast over the frame's bins (the last axis of ``p_ref``)."""
    e = np.asarray(e, dtype=np.float64)[..., None]
    return (1.5 + 2.0 * h) * 2.0 ** -23 * p_ref + 2.0 * np.sqrt(p_ref) * e + e * e


def n_frames_of(n_samples, hop):
    return 1 + n_samples // hop


def frames_of(clip, hop):
    """The centred, zero-padded frames of a clip: frame t starts at t * hop - 1024; (n_frames, 2048) float32."""
    clip = np.asarray(clip)
    assert clip.dtype == np.float32 and clip.ndim == 1
    n = len(clip)
    padded = np.concatenate([np.zeros(N_FFT // 2, np.float32), clip, np.zeros(N_FFT // 2 + hop, np.float32)])
    return np.stack([padded[t * hop:t * hop + N_FFT] for t in range(n_frames_of(n, hop))])


def project32(pw, basis, lo, hi, smallest=False):
    """The kernels' projection (csrc/mel_body.h): ``pw`` (1025, ...) float32 power values, ``basis`` (M, 1025) float32,
    ``lo``/``hi`` (M) -> (M, ...) float32.  Per filter, for q = 0..3: acc_q = +0.0, then acc_q = acc_q + float32(row[f] *
    pw[f]) for f = lo + q, lo + q + 4, ... < hi ascending; the result is (acc_0 + acc_1) + (acc_2 + acc_3).
    ``smallest``: also return the smallest non-zero magnitude among all products and sums formed."""
    pw, basis = np.asarray(pw), np.asarray(basis)
    assert pw.dtype == np.float32 and basis.dtype == np.float32 and pw.shape[0] == N_BINS and basis.shape[1] == N_BINS
    out = np.zeros((basis.shape[0],) + pw.shape[1:], dtype=np.float32)
    least = [np.inf]

    def seen(v):
        if smallest:
            mag = np.abs(v[v != 0])
            if mag.size:
                least[0] = min(least[0], float(mag.min()))
        return v

    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(basis.shape[0]):
            acc = [np.zeros(pw.shape[1:], dtype=np.float32) for _ in range(4)]
            for q in range(4):
                for f in range(int(lo[m]) + q, int(hi[m]), 4):
                    acc[q] = seen(acc[q] + seen(basis[m, f] * pw[f]))
            out[m] = seen(seen(acc[0] + acc[1]) + seen(acc[2] + acc[3]))
    assert out.dtype == np.float32
    return (out, least[0]) if smallest else out


# ---- the designed clips ---------------------------------------------------------------------------------------------------
def impulse_sample(n_samples, hop, position):
    """(sample index, frame) that put a clip's single non-zero sample at window position ``position`` of a frame: of the
    first WHOLE frame (one that lies inside the clip) where the clip has one, else of the first frame that reaches it
    there; None where no frame of the clip does."""
    starts = [t * hop - N_FFT // 2 for t in range(n_frames_of(n_samples, hop))]
    whole = [t for t, s in enumerate(starts) if s >= 0 and s + N_FFT <= n_samples]
    for t in whole or range(len(starts)):
        if 0 <= starts[t] + position < n_samples:
            return starts[t] + position, t
    return None


def designed_clips(n_samples, hop):
    """The clips of one shape: (clips (B, n_samples) float32, families: B names, impulses: [(clip, frame, position)])."""
    key = ("clips", n_samples, hop)
    if key not in _CACHE:
        rng = np.random.default_rng(1025 * n_samples + hop)
        n = np.arange(n_samples, dtype=np.float64)
        clips, families, impulses = [], [], []
        for position in IMPULSE_POSITIONS:
            at = impulse_sample(n_samples, hop, position)
            if at is None:
                continue
            clip = np.zeros(n_samples, dtype=np.float32)
            clip[at[0]] = IMPULSE_LEVEL
            impulses.append((len(clips), at[1], position))
            clips.append(clip)
            families.append("impulse")
        for k0 in TONE_BINS:
            clips.append((0.5 * np.cos(2.0 * np.pi * k0 * n / N_FFT + 0.3)).astype(np.float32))
            families.append("tone")
        for scale in NOISE_SCALES:
            clips.append((rng.standard_normal(n_samples) * scale).astype(np.float32))
            families.append(f"noise {scale:g}")
        clips.append(np.zeros(n_samples, dtype=np.float32))
        families.append("zero")
        clips = np.stack(clips)
        clips.setflags(write=False)
        _CACHE[key] = (clips, families, impulses)
    return _CACHE[key]


def designed_frames(n_samples, hop):
    """Every frame of every designed clip of a shape: (B, n_frames, 2048) float32."""
    key = ("frames", n_samples, hop)
    if key not in _CACHE:
        _CACHE[key] = np.stack([frames_of(c, hop) for c in designed_clips(n_samples, hop)[0]])
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def reference(n_samples, hop):
    """(P_ref (B, n_frames, 1025) float64, e (B, n_frames)) of a shape's designed clips, computed once."""
    key = ("ref", n_samples, hop)
    if key not in _CACHE:
        frames = designed_frames(n_samples, hop)
        _CACHE[key] = (dft_power64(frames), transform_error(frames))
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def projection_clip(n_samples, hop):
    """Index of the clip whose power spectrum the projection tests use: the noise clip of scale 0.1."""
    return designed_clips(n_samples, hop)[1].index("noise 0.1")


# ---- the designed bases ---------------------------------------------------------------------------------------------------
def identity_basis():
    """1025 one-bin filters: basis[m, m] = 1, lo[m] = m, hi[m] = m + 1.  The projection then returns pw itself:
    lane 0 of a filter's four adds 1.0f * pw[m] to +0.0, the others add nothing, (pw + 0) + (0 + 0) = pw."""
    idx = np.arange(N_BINS, dtype=np.int32)
    return np.eye(N_BINS, dtype=np.float32), idx.copy(), idx + 1


def _filter_ranges():
    """(lo, hi) of the designed filters: every width 0..72 at every lo % 4, lo = 0 for the even widths at residue 0 and
    hi = 1025 for the odd widths at the residue that allows it; then the one filter over all 1025 bins."""
    rng = np.random.default_rng(72)
    ranges = []
    for width in range(MAX_WIDTH + 1):
        for residue in range(4):
            if residue == 0 and width % 2 == 0:
                lo = 0
            elif width % 2 == 1 and (N_BINS - width) % 4 == residue:
                lo = N_BINS - width
            else:
                lo = residue + 4 * int(rng.integers(0, (N_BINS - width - residue) // 4 + 1))
            assert lo % 4 == residue and 0 <= lo and lo + width <= N_BINS
            ranges.append((lo, lo + width))
    ranges.append((0, N_BINS))
    return ranges


def _basis_of(ranges, seed):
    """Weights uniform in +-[2^-10, 1] inside [lo, hi), 1e30 outside."""
    rng = np.random.default_rng(seed)
    basis = np.full((len(ranges), N_BINS), FILL, dtype=np.float32)
    for m, (lo, hi) in enumerate(ranges):
        weights = rng.uniform(2.0 ** -10, 1.0, hi - lo) * rng.choice([-1.0, 1.0], hi - lo)
        basis[m, lo:hi] = weights.astype(np.float32)
    lo, hi = (np.array(v, dtype=np.int32) for v in zip(*ranges))
    return basis, lo, hi


def designed_bases():
    """name -> (basis, lo, hi): 293 filters (every designed range; the last group of sixteen holds five), 304 filters
    (19 whole groups: eleven more ranges that end at bin 1025 or start at bin 0) and one filter (all 1025 bins)."""
    if "bases" not in _CACHE:
        ranges = _filter_ranges()
        more = [(N_BINS - w, N_BINS) for w in (0, 2, 4, 6, 33, 70, 72)] + [(0, w) for w in (1, 3, 31, 71)]
        assert len(ranges) == 293 and len(ranges + more) == 304
        _CACHE["bases"] = {"293 filters": _basis_of(ranges, 293), "304 filters": _basis_of(ranges + more, 304),
                           "1 filter": _basis_of([(0, N_BINS)], 1)}
    return _CACHE["bases"]
