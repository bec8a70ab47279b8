"""SPEC.md 1.12 restated in NumPy for the speed perturbation's tests (test_speed_host.py, test_gpu_speed.py), on the
resampler's restatement (resample_restatement.causal): a clip with a design is y[m] = z[m + D] on that design, a clip
without one its own bits and +0.0 behind them."""
import numpy as np

import resample_restatement as RS


def zero_from(n_in, table):
    """ceil((n_in + Hs) * up / down): from this output on every tap of every sample meets a zero."""
    return -(-(int(n_in) + int(table.history)) * int(table.up) // int(table.down))


def perturb(x, table, n_out):
    """One clip ``x`` (1-D float32 or int16) -> float32 (n_out,).  ``table`` None: the unperturbed clip."""
    x, n_out = np.asarray(x), int(n_out)
    if table is None:
        out = np.zeros(n_out, dtype=np.float32)
        m = min(len(x), n_out)
        if x.dtype == np.int16:
            out[:m] = x[:m].astype(np.float32) * np.float32(2.0 ** -15)
        else:
            assert x.dtype == np.float32
            out[:m].view(np.uint32)[:] = x[:m].view(np.uint32)
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        return RS.causal(x, table, table.delay, n_out)


def perturb_batch(x, tables, rows, n_out):
    """``x`` (B, n_in) float32 or int16, ``tables`` the bank's designs, ``rows`` B integers or None (row 0 everywhere) ->
    float32 (B, n_out).  A row below 0 is an unperturbed clip; a row at or above len(tables) is clamped to the last."""
    x = np.asarray(x)
    assert x.ndim == 2 and len(tables) >= 1
    B = x.shape[0]
    rows = np.zeros(B, dtype=np.int64) if rows is None else np.broadcast_to(np.asarray(rows, dtype=np.int64), (B,))
    out = np.zeros((B, int(n_out)), dtype=np.float32)
    for b in range(B):
        table = None if rows[b] < 0 else tables[int(min(rows[b], len(tables) - 1))]
        out[b] = perturb(x[b], table, n_out)
    return out
