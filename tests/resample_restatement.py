"""SPEC.md 1.8 restated in NumPy for the resampler's tests (test_resample_host.py, test_gpu_resample.py): the causal
sample z[m] summed tap by tap in the stated order, vectorised over the outputs, float64 without FMA, rounded once to float32."""
import numpy as np


def widen(x):
    """Samples as the kernels widen them: int16 times 2^-15 as float32 (exact), then float64."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = x.astype(np.float32) * np.float32(2.0 ** -15)
    assert x.dtype == np.float32 and x.ndim == 1
    return x.astype(np.float64)


def causal(x, table, first, count, origin=0):
    """z[first], ..., z[first + count - 1] of the signal whose sample 0 is ``x[origin]`` (x: 1-D float32 or int16); what
    lies before ``x[0]`` or behind its end is +0.0, and still multiplied and added."""
    x64 = widen(x)
    taps, up, down = np.asarray(table.taps, dtype=np.float64), int(table.up), int(table.down)
    K, n = len(taps), len(x64)
    p = np.arange(first, first + count, dtype=np.int64) * down
    k0, i0 = p % up, p // up + origin
    acc = np.zeros(count, dtype=np.float64)                     # +0.0
    for j in range(-(-K // up)):                                # k = k0, k0 + up, ... < K, in this order
        k = k0 + j * up
        i = i0 - j
        xv = np.where((i >= 0) & (i < n), x64[np.clip(i, 0, n - 1)], 0.0)
        acc = np.where(k < K, acc + taps[np.minimum(k, K - 1)] * xv, acc)
    return acc.astype(np.float32)


def batch(x, table, n_out=None):
    """The batch form: y[m] = z[m + D], resample_poly's length by default."""
    if n_out is None:
        n_out = -(-len(x) * table.up // table.down)
    return causal(x, table, table.delay, n_out)


def stream(x, table):
    """The streamed form over the whole blocks of x: z[0 .. blocks * up)."""
    blocks = len(x) // table.down
    return causal(x[:blocks * table.down], table, 0, blocks * table.up)


def stream_cut(x, table, cuts):
    """The streamed form pushed in pieces of ``cuts`` blocks: every push sees only [history | its blocks] and no position,
    as the kernel does, the history carried as float32.  Returns (samples, final history)."""
    down, Hs = table.down, table.history
    x32 = widen(x).astype(np.float32)
    hist = np.zeros(Hs, dtype=np.float32)
    outs, pos = [np.zeros(0, dtype=np.float32)], 0
    for kb in cuts:
        run = np.concatenate([hist, x32[pos:pos + kb * down]])
        outs.append(causal(run, table, 0, kb * table.up, origin=Hs))
        hist = run[len(run) - Hs:]
        pos += kb * down
    return np.concatenate(outs), hist
