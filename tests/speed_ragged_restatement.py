"""SPEC.md 1.18 restated in NumPy for the ragged speed perturbation's tests (test_speed_ragged_host.py,
test_gpu_speed_ragged.py), on the restatement of 1.12 (speed_restatement.perturb) unchanged: per clip that restatement on
``audio[b, :n_b]`` alone at ``n_out = n'_b``, then +0.0."""
import numpy as np

import speed_restatement as SR

HOP = 160


def clamp_samples(clip_samples, n_in):
    """n_b = clamp(clip_samples[b], 0, n_in)."""
    return np.clip(np.asarray(clip_samples, dtype=np.int64), 0, int(n_in))


def new_length(n_b, table, n_out):
    """n'_b in Python integers: min(ceil(n_b * up / down), n_out) with a design, min(n_b, n_out) without one."""
    n_b, n_out = int(n_b), int(n_out)
    if table is None:
        return min(n_b, n_out)
    return min(-(-n_b * int(table.up) // int(table.down)), n_out)


def table_of(tables, row):
    """The design of a row under 1.12's rules: below 0 none, at or above len(tables) the last."""
    return None if row < 0 else tables[int(min(row, len(tables) - 1))]


def perturb_ragged(x, clip_samples, tables, rows, n_out, time_bins):
    """``x`` (B, n_in) float32 or int16, ``clip_samples`` B integers, ``tables`` the bank's designs, ``rows`` B integers or
    None (row 0 everywhere) -> ``(out float32 (B, n_out), samples int32 (B,), bins int32 (B,))``.  What lies behind a clip in
    its row is never looked at."""
    x = np.asarray(x)
    assert x.ndim == 2 and len(tables) >= 1
    B, n_in = x.shape
    rows = np.zeros(B, dtype=np.int64) if rows is None else np.broadcast_to(np.asarray(rows, dtype=np.int64), (B,))
    out = np.zeros((B, int(n_out)), dtype=np.float32)
    samples = np.zeros(B, dtype=np.int32)
    for b, n_b in enumerate(clamp_samples(clip_samples, n_in)):
        table = table_of(tables, rows[b])
        samples[b] = new_length(n_b, table, n_out)
        if samples[b]:
            out[b, :samples[b]] = SR.perturb(x[b, :n_b], table, samples[b])
    bins = np.minimum(-(-samples.astype(np.int64) // HOP), int(time_bins)).astype(np.int32)
    return out, samples, bins
