"""The two FIR operations of the audio chain by their definitions, for the tests of the resampler (SPEC.md 1.8) and of the
reverberation (SPEC.md 1.11): test_fir_definition_host.py, test_gpu_resample.py, test_gpu_resample_range.py and
test_gpu_reverb.py.  Neither restatement (resample_restatement.py, reverb_restatement.py) is used here beyond `widen`, and
no sum is taken tap by tap in the kernels' order.

Resampler.  The samples widened as the kernels widen them, zero-stuffed by ``up`` into ``np.longdouble``,
``full = np.convolve(stuffed, taps)``, then ``z[m] = full[m * down]``, zero past the end; the batch form is ``z[m + delay]``.
``np.convolve`` costs ``len(stuffed) * K`` multiply-adds whatever the zeros, which at 44.1 kHz (160 phases of 9262 taps) or
with 4096 phases is minutes per row; above `LITERAL_MACS` the same ``full`` is built column by column instead: written as
rows of ``up`` positions, its column r is ``np.convolve(x, taps[r::up])``, since every other product of the full sum has a
stuffed zero in it.  The sums are still np.convolve's, and ``z[m] = full[m * down]`` is still read off ``full``.
`test_fir_definition_host.py` shows that the two forms give the same values.

Reverberation.  ``np.convolve(x, h[:len])`` in ``np.longdouble``.

``S`` is the same sum over absolute values, and the bound per output is derived, not measured:

    resampler  |got - ref| <= 2^-24 |ref| + 2 T 2^-52 S + 2^-149,   T = ceil(K / up)
    reverb     |got - ref| <= 2^-24 |ref| +   len 2^-52 S + 2^-149

A float64 sum over at most T taps with a rounded product and a rounded add per tap is off by 2 T 2^-53 S to first order; the
factor 2 covers the higher orders; one rounding to float32 follows (2^-24 |ref|, or half the smallest subnormal).  The
reverberation's products are exact and fused into the add, one rounding per tap.  Where ``np.longdouble`` is no wider than
float64 (`WIDE` false) the reference carries the same error as the sum under test, and the middle term is doubled.
An output whose reference is NaN or infinite is compared by class, not by bound."""
from types import SimpleNamespace

import numpy as np

from resample_restatement import widen

LD = np.longdouble
WIDE = bool(np.finfo(LD).eps < np.finfo(np.float64).eps)
MIDDLE = 1.0 if WIDE else 2.0
LITERAL_MACS = 1 << 27              # up to here `full` is np.convolve of the stuffed signal itself


# ---- resampler -----------------------------------------------------------------------------------------------------------
def full_literal(x, taps, up, pos):
    """``np.convolve(stuffed, taps)[pos]``, zero past the end."""
    stuffed = np.zeros(len(x) * up, dtype=LD)
    stuffed[::up] = x
    full = np.convolve(stuffed, taps)
    return np.where(pos < len(full), full[np.minimum(pos, len(full) - 1)], LD(0))


def full_by_columns(x, taps, up, pos):
    """The same values with the stuffed zeros' products left out: ``full`` seen as rows of ``up`` positions has
    ``np.convolve(x, taps[r::up])`` as its column r."""
    q, r = np.divmod(pos, up)
    order = np.argsort(r, kind="stable")
    cols, starts = np.unique(r[order], return_index=True)
    out = np.zeros(len(pos), dtype=LD)
    for col, a, b in zip(cols, starts, list(starts[1:]) + [len(pos)]):
        sub = taps[col::up]
        if len(sub):
            column = np.convolve(x, sub)
            sel = order[a:b]
            out[sel] = np.where(q[sel] < len(column), column[np.minimum(q[sel], len(column) - 1)], LD(0))
    return out


def _full_at(x, taps, up, pos):
    with np.errstate(invalid="ignore", over="ignore"):
        if len(x) * up * len(taps) <= LITERAL_MACS:
            return full_literal(x, taps, up, pos)
        return full_by_columns(x, taps, up, pos)


def resample(x, table, first, count):
    """``(z, S)`` for the outputs ``first .. first + count - 1`` of the causal run over ``x`` (1-D float32 or int16), both
    ``np.longdouble``: the streamed form is ``first = 0``, the batch form ``first = delay``."""
    xw, taps = widen(x).astype(LD), np.asarray(table.taps, dtype=np.float64).astype(LD)
    pos = np.arange(first, first + count, dtype=np.int64) * int(table.down)
    return _full_at(xw, taps, int(table.up), pos), _full_at(np.abs(xw), np.abs(taps), int(table.up), pos)


def resample_bound(ref, S, table):
    T = -(-len(table.taps) // int(table.up))
    return LD(2.0 ** -24) * np.abs(ref) + LD(MIDDLE * 2 * T * 2.0 ** -52) * S + LD(2.0 ** -149)


# ---- reverberation -------------------------------------------------------------------------------------------------------
def reverb(x, h, n_out=None):
    """``(y, S)``: ``np.convolve(x, h)`` cut or zero-padded to ``n_out`` (default ``len(x)``), and the same of the absolute
    values.  ``h`` is the row up to its length, all of it used."""
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == np.float32 and h.dtype == np.float32 and x.ndim == 1 and h.ndim == 1 and len(h) >= 1
    n_out = len(x) if n_out is None else int(n_out)
    xw, hw = x.astype(LD), h.astype(LD)

    def cut(full):
        out = np.zeros(n_out, dtype=LD)
        m = min(n_out, len(full))
        out[:m] = full[:m]
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        return cut(np.convolve(xw, hw)), cut(np.convolve(np.abs(xw), np.abs(hw)))


def reverb_bound(ref, S, length):
    return LD(2.0 ** -24) * np.abs(ref) + LD(MIDDLE * int(length) * 2.0 ** -52) * S + LD(2.0 ** -149)


# ---- the comparison ------------------------------------------------------------------------------------------------------
def worst(got, ref, bound):
    """The largest ``err / bound`` over the outputs with a finite reference (0.0 if there is none); an output of another
    class than its reference -- NaN against a number, the wrong infinity -- counts as infinitely far off."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape == bound.shape, (got.dtype, got.shape, ref.shape)
    finite = np.isfinite(ref)
    nan, inf = np.isnan(ref), np.isinf(ref)
    if (np.isnan(got) != nan).any() or (got[inf] != ref[inf]).any():
        return float("inf")
    if not finite.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got[finite].astype(LD) - ref[finite]) / bound[finite]
    return float(ratio.max())


def check(got, ref, bound, what):
    """Print the worst ``err / bound`` and assert that no output lies outside its bound; returns the ratio."""
    w = worst(got, ref, bound)
    print(f"{what}: worst err / bound = {w:.4f}")
    assert w <= 1.0, f"{what}: an output lies {w:.3f} bounds from the definition"
    return w


# ---- the inputs that the host and the GPU tests share --------------------------------------------------------------------
# (up, down, K) of the tables beyond the packaged designs (test_gpu_resample_range.py says what each one reaches)
RANGE_TABLES = ((1, 2, 1100), (3, 2, 2000), (5, 4, 10), (7, 3, 5), (2, 1, 1), (640, 441, 19840), (4096, 4095, 20480))
RANGE_N_OUT = 2 * 2048 + 37         # two tiles of the resampler and an odd remainder
# row lengths at the edges of the reverberation's tap loop: groups of 8, chunks of 1024, one short of the 16384 a row can hold
REVERB_LENGTHS = (7, 8, 9, 1023, 1024, 1025, 1031, 1032, 1033, 2047, 2049, 16383)
REVERB_TAPS = 16384
REVERB_N = 2100
REVERB_CUTS = (1, 2047, REVERB_N - 2048)
REVERB_N_OUT = REVERB_N + REVERB_TAPS + 1  # the batch form with the whole tail of the longest row behind the clip, and zeros


def range_table(up, down, K, delay=0):
    """Seeded Gaussian taps without decay -- every tap carries weight -- scaled so that an output is of its input's order."""
    taps = np.random.default_rng(100003 * up + K).standard_normal(K) / np.sqrt(max(1.0, K / up))
    return SimpleNamespace(taps=taps, up=up, down=down, delay=delay, history=(K - 1) // up)


def range_delays(table):
    """0, one in between, and the last delay the ABI accepts: delay * down <= K - 1."""
    last = (len(table.taps) - 1) // table.down
    return sorted({0, last // 2, last})


def pcm_noise(n_rows, n, seed, dtype):
    """Rows of seeded noise under a level ramp; row 2 begins with exact zeros, and row 1 is 60 dB down in its middle third, so
    that a bound taken from a clip's loudest sample would say nothing there."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, n)) * np.linspace(0.02, 0.6, n)[None, :]
    if n_rows > 2:
        x[2, :n // 7] = 0.0
    if n_rows > 1:
        x[1, n // 3:2 * n // 3] *= 1e-3
    if dtype == np.int16:
        return np.clip(np.round(x * 8192), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def range_input(table, dtype, n_rows=3):
    """Clips for `RANGE_N_OUT` outputs at delay 0: a little short of them, so that the last outputs run off the end."""
    n_in = max(8, RANGE_N_OUT * table.down // table.up - 5)
    return pcm_noise(n_rows, n_in, 7 * table.up + len(table.taps), dtype)


def reverb_edge_bank():
    """(bank (12, 16384) float32, lengths int32): Gaussian rows without decay, h[0] = 1, and 1e30 behind each row's length."""
    rng = np.random.default_rng(1611)
    bank = (rng.standard_normal((len(REVERB_LENGTHS), REVERB_TAPS)) * 0.05).astype(np.float32)
    bank[:, 0] = 1.0
    lengths = np.array(REVERB_LENGTHS, dtype=np.int32)
    for r, n in enumerate(lengths):
        bank[r, n:] = np.float32(1e30)
    return bank, lengths


def reverb_edge_audio():
    """One clip per row of `reverb_edge_bank`."""
    return (np.random.default_rng(1612).standard_normal((len(REVERB_LENGTHS), REVERB_N)) * 0.1).astype(np.float32)
