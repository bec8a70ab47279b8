"""SPEC.md 1.11 restated in NumPy for the reverberation tests (test_reverb_host.py, test_gpu_reverb.py): per output
``acc = +0.0; for k ascending: acc = acc + h[k] * x[i - k]`` in float64, one rounding to float32 -- a loop over k on whole
arrays.  The product of two float32 values is exact in float64, so NumPy's multiply-then-add gives the bits of the
kernels' fused multiply-add.  Samples outside the signal are +0.0 and are multiplied and added like any other."""
import numpy as np


def row_length(lengths, r, K):
    """len_r = clamp(rir_len[r], 1, K); None means K everywhere."""
    return K if lengths is None else int(np.clip(int(lengths[r]), 1, K))


def push_count(counts, b, n_cols):
    """c_b = clamp(count[b], 0, n_cols): the samples of stream b that a push of ``n_cols`` columns takes; None means n_cols."""
    return n_cols if counts is None else int(np.clip(int(counts[b]), 0, n_cols))


def convolve(x, h, n_out=None, history=None):
    """One signal ``x`` (1-D float32) against taps ``h`` (1-D float32, all of them used) -> float32 (n_out,).  ``history``:
    float32 samples in front of x[0] (the last one is x[-1]); further back, and at or past the end of x, +0.0."""
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == np.float32 and h.dtype == np.float32 and x.ndim == 1 and h.ndim == 1 and len(h) >= 1
    n, K = len(x), len(h)
    n_out = n if n_out is None else int(n_out)
    front = K - 1
    ext = np.zeros(front + max(n, n_out) + K, dtype=np.float64)           # ext[front + i] = x[i]
    ext[front:front + n] = x.astype(np.float64)
    if history is not None and front:
        hist = np.asarray(history, dtype=np.float32)[-front:]
        ext[front - len(hist):front] = hist.astype(np.float64)
    hd = h.astype(np.float64)
    acc = np.zeros(n_out, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):                                                # k ascending
            acc = acc + hd[k] * ext[front - k:front - k + n_out]
        return acc.astype(np.float32)


def reverb(audio, bank, lengths=None, rows=None, n_out=None):
    """The batch form: ``audio`` (B, n) float32, ``bank`` (M, K) float32 -> float32 (B, n_out).  A row below 0 is dry: the
    clip's bits, +0.0 behind it; a row at or above M is clamped."""
    audio, bank = np.asarray(audio), np.asarray(bank)
    assert audio.dtype == np.float32 and audio.ndim == 2 and bank.dtype == np.float32 and bank.ndim == 2
    B, n = audio.shape
    M, K = bank.shape
    n_out = n if n_out is None else int(n_out)
    rows = np.zeros(B, dtype=np.int64) if rows is None else np.broadcast_to(np.asarray(rows, dtype=np.int64), (B,))
    out = np.zeros((B, n_out), dtype=np.float32)
    for b in range(B):
        if rows[b] < 0:
            m = min(n, n_out)
            out[b, :m].view(np.uint32)[:] = audio[b, :m].view(np.uint32)
            continue
        r = int(min(rows[b], M - 1))
        out[b] = convolve(audio[b], bank[r, :row_length(lengths, r, K)], n_out)
    return out


def new_state(K):
    """A stream's start: K - 1 zeros."""
    return np.zeros(K - 1, dtype=np.float32)


def stream(x, bank, state, lengths=None, row=0):
    """One push of one stream: ``x`` (1-D float32, any length), ``state`` its last K - 1 input samples ->
    ``(y float32, the new state)``."""
    x, bank = np.asarray(x), np.asarray(bank)
    assert x.dtype == np.float32 and x.ndim == 1 and state.dtype == np.float32 and len(state) == bank.shape[1] - 1
    M, K = bank.shape
    if len(x) == 0:
        return np.zeros(0, dtype=np.float32), state.copy()
    if row < 0:
        y = x.copy()
    else:
        r = int(min(row, M - 1))
        y = convolve(x, bank[r, :row_length(lengths, r, K)], len(x), history=state)
    return y, np.concatenate([state, x])[len(state) + len(x) - (K - 1):].copy()


def stream_cut(x, bank, cuts, lengths=None, row=0, state=None):
    """The same stream pushed in pieces of ``cuts`` samples; ``row`` a number or one per push.
    -> ``(y, the final state)``."""
    state = new_state(bank.shape[1]) if state is None else state
    rows = np.broadcast_to(np.asarray(row, dtype=np.int64), (len(cuts),))
    parts, at = [np.zeros(0, dtype=np.float32)], 0
    for c, r in zip(cuts, rows):
        y, state = stream(x[at:at + c], bank, state, lengths, int(r))
        parts.append(y)
        at += c
    assert at == len(x)
    return np.concatenate(parts), state
