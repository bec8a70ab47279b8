"""SPEC.md 1.10 restated in NumPy for the noise mixer's tests (test_mix_host.py, test_gpu_mix.py): the row power summed in
the stated order -- 256 strided partial sums, then the tree -- the zero-filled shift, the wrapped noise row, the gain with
IEEE division and square root, float64 without FMA throughout and one rounding to float32."""
import numpy as np

LANES = 256


def power(u):
    """P of every row of ``u`` (..., n): float32 (widened) or float64 in, float64 out.  A lane's missing samples add +0.0,
    which leaves a partial sum as it is: it starts at +0.0 and a square is never -0.0."""
    u = np.asarray(u)
    assert u.dtype in (np.float32, np.float64)
    u = u.astype(np.float64)
    lead, n = u.shape[:-1], u.shape[-1]
    steps = -(-n // LANES)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.zeros(lead + (steps * LANES,), dtype=np.float64)
        sq[..., :n] = u * u
        sq = sq.reshape(lead + (steps, LANES))
        p = np.zeros(lead + (LANES,), dtype=np.float64)
        for k in range(steps):                                  # k = 0, 256, ... ascending
            p = p + sq[..., k, :]
        s = LANES // 2
        while s >= 1:
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
    return p[..., 0]


def shifted(audio, shift, scale):
    """x of the batch form: ``audio`` (B, n) float32 -> float64 (B, n), the product exact, +0.0 where the shift leaves none."""
    audio = np.asarray(audio)
    assert audio.dtype == np.float32 and audio.ndim == 2
    B, n = audio.shape
    s = np.clip(np.asarray(shift, dtype=np.int64), -n, n)
    a = np.asarray(scale, dtype=np.float32).astype(np.float64)
    j = np.arange(n, dtype=np.int64)[None, :] - s[:, None]
    inside = (j >= 0) & (j < n)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = a[:, None] * np.take_along_axis(audio.astype(np.float64), np.clip(j, 0, n - 1), axis=1)
    return np.where(inside, prod, 0.0)


def noise_rows(noise, rows, offsets, n):
    """v of the batch form: float64 (B, n), the row clamped, the offset taken modulo L, the row wrapped as often as needed."""
    noise = np.asarray(noise)
    assert noise.dtype == np.float32 and noise.ndim == 2
    M, L = noise.shape
    r = np.clip(np.asarray(rows, dtype=np.int64), 0, M - 1)
    o = np.mod(np.asarray(offsets, dtype=np.int64), L)
    idx = (o[:, None] + np.arange(n, dtype=np.int64)[None, :]) % L
    return noise[r[:, None], idx].astype(np.float64)


def _per_clip(value, B, dtype):
    return np.broadcast_to(np.asarray(value, dtype=dtype), (B,)).copy()


def mix(audio, noise, ratio, rows=0, offsets=0, shift=0, scale=1.0):
    """The batch form -> ``(y float32 (B, n), g float64 (B), powers float64 (B, 2))``."""
    audio = np.asarray(audio)
    B, n = audio.shape
    q = _per_clip(ratio, B, np.float64)
    x = shifted(audio, _per_clip(shift, B, np.int64), _per_clip(scale, B, np.float32))
    v = noise_rows(noise, _per_clip(rows, B, np.int64), _per_clip(offsets, B, np.int64), n)
    Px, Pv = power(x), power(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        noisy = (q > 0) & (Pv > 0)
        g = np.where(noisy, np.sqrt((Px * q) / np.where(noisy, Pv, 1.0)), 0.0)
        gv = g[:, None] * np.where(noisy[:, None], v, 0.0)      # the product rounded, then the sum
        y = np.where(noisy[:, None], x + gv, x).astype(np.float32)
    return y, g, np.stack([Px, Pv], axis=1)


def stream(x, noise, gain, row=0, scale=1.0, pos=0):
    """One stream's samples ``x`` (1-D float32) from noise position ``pos`` -> ``(y float32, position behind them)``."""
    x = np.asarray(x)
    noise = np.asarray(noise)
    assert x.dtype == np.float32 and x.ndim == 1 and noise.dtype == np.float32 and noise.ndim == 2
    M, L = noise.shape
    r = int(np.clip(int(row), 0, M - 1))
    p = int(pos) % L
    a = np.float64(np.float32(scale))
    g = np.float64(gain)
    with np.errstate(invalid="ignore", over="ignore"):
        ax = a * x.astype(np.float64)
        if g == 0:
            y = ax.astype(np.float32)
        else:
            v = noise[r, (p + np.arange(len(x), dtype=np.int64)) % L].astype(np.float64)
            y = (ax + g * v).astype(np.float32)
    return y, (p + len(x)) % L


def stream_cut(x, noise, gain, cuts, row=0, scale=1.0, pos=0):
    """The same stream pushed in pieces of ``cuts`` samples: a push sees its samples and the position, nothing else."""
    parts, at = [np.zeros(0, dtype=np.float32)], 0
    for c in cuts:
        y, pos = stream(x[at:at + c], noise, gain, row, scale, pos)
        parts.append(y)
        at += c
    assert at == len(x)
    return np.concatenate(parts), pos
