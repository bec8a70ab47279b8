"""The spike encoder's definition on the host (SPEC.md 1.2-1.3): the resize of oracle/ref_numpy.py and oracle/lsm_oracle.c
against scipy.ndimage.zoom itself over a whole square of (columns, time bins), the widths included whose last coordinate
overshoots the input (SciPy answers 0.0 there), and the latch restatement of tests/encoder_restatement.py against the
reference's golden vectors.  Then the definition's teeth: three wrong encoders it must tell apart on the very inputs the
GPU tests use (tests/test_gpu_encoder_range.py).  CPU only."""
import os
import sys

import numpy as np
import pytest
from scipy.ndimage import zoom

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_restatement as ER  # noqa: E402
from oracle import ref_numpy as O  # noqa: E402

LO, HI = 2, 130                      # the swept square [LO, HI]^2
N_OVERSHOOT = 568                    # pairs of it whose last coordinate overshoots (237 in [2, 96]^2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _rows(rng, nc, dt):
    """Three rows in [0, 1] holding an exact 0.0 and 1.0: already normalised, so `(x - 0) / (1 - 0 + 1e-8)` is all the C
    entry points add before the resize."""
    x = rng.random((3, nc))
    x[0, 0], x[1, nc - 1] = 0.0, 1.0
    return x.astype(dt)


def _scipy_chain(x, tb):
    """create_dataset.py:62-78 with SciPy itself."""
    dt = x.dtype.type
    lo, hi = x.min(), x.max()
    norm = (x - lo) / (dt(hi - lo) + dt(1e-8))
    assert norm.dtype == x.dtype
    z = zoom(norm, (1, tb / x.shape[1]), order=1) if x.shape[1] != tb else norm
    assert z.shape[1] == tb and z.dtype == x.dtype
    return norm, z[:, :tb]


def _check_pair(oracle_c, rng, nc, tb, dt):
    x = _rows(rng, nc, dt)
    norm, z = _scipy_chain(x, tb)
    got_np = O.zoom_linear(norm, tb)
    got_c = oracle_c.normalise_resize(x, tb)
    assert got_np.dtype == got_c.dtype == z.dtype
    assert np.array_equal(_bits(got_np), _bits(z)), (nc, tb, dt.__name__, "ref_numpy.zoom_linear")
    assert np.array_equal(_bits(got_c), _bits(z)), (nc, tb, dt.__name__, "orc_normalise_resize")
    if ER.overshoots(nc, tb):
        assert not _bits(z[:, tb - 1]).any() and z[:, :tb - 1].any(), (nc, tb)     # +0.0 in the last bin, there alone


def test_resize_equals_scipy_over_the_whole_square_float64(oracle_c):
    """Every (ncols, time_bins) of [2, 130]^2 with ncols != time_bins, float64, byte for byte; the overshooting pairs are
    counted from the inequality so that the sweep cannot lose them."""
    rng = np.random.default_rng(1)
    n_over = 0
    for nc in range(LO, HI + 1):
        for tb in range(LO, HI + 1):
            if nc == tb:
                continue
            n_over += ER.overshoots(nc, tb)
            _check_pair(oracle_c, rng, nc, tb, np.float64)
    assert n_over == N_OVERSHOOT
    for pair in ((105, 100), (58, 100), (30, 8), (26, 12), (8, 26), (16, 30), (32, 31), (31, 30)):
        assert ER.overshoots(*pair), pair
    for pair in ((98, 100), (101, 100), (100, 100), (33, 70), (64, 31)):           # shapes of the earlier tests
        assert not ER.overshoots(*pair), pair


def test_resize_equals_scipy_float32(oracle_c):
    """float32 (the mel branch: float32 normalise, double interpolation, cast back): every overshooting pair of the square
    and every seventh of the others."""
    rng = np.random.default_rng(2)
    n_over = n_rest = 0
    for nc in range(LO, HI + 1):
        for tb in range(LO, HI + 1):
            if nc == tb:
                continue
            over = ER.overshoots(nc, tb)
            if over or (nc * 131 + tb) % 7 == 0:
                n_over += over
                n_rest += not over
                _check_pair(oracle_c, rng, nc, tb, np.float32)
    assert n_over == N_OVERSHOOT and n_rest > 2000


def test_resize_equals_scipy_for_100_bins_up_to_3000_columns(oracle_c):
    """The reference's own bin count against every width a clip can have: 153 of them overshoot."""
    rng = np.random.default_rng(3)
    over = [nc for nc in range(2, 3001) if ER.overshoots(nc, 100)]
    assert len(over) == 153
    assert [nc for nc in over if nc < 260] == [14, 27, 53, 58, 105, 108, 115, 122, 209, 212, 215, 226, 229, 232, 243, 246]
    for nc in range(2, 3001):
        if nc != 100:
            _check_pair(oracle_c, rng, nc, 100, np.float64)
    for nc in over:
        _check_pair(oracle_c, rng, nc, 100, np.float32)


@pytest.mark.parametrize("nc,tb", [(105, 100), (30, 8), (8, 26)])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_resize_of_nan_and_inf_rows_at_an_overshooting_width(oracle_c, nc, tb, dt):
    """SciPy's 0.0 for a coordinate outside the input does not look at the row: NaN and +-Inf rows end in +0.0 too.  The
    restatement follows, in every bin of a NaN row and in every finite bin of an Inf row, and so does a whole NaN clip
    through the C entry points (one NaN makes min and max NaN, hence every normalised value; the last bin is still 0.0)."""
    rng = np.random.default_rng(nc)
    x = rng.random((6, nc)).astype(dt)
    x[0, :] = np.nan
    x[1, nc - 1] = np.nan
    x[2, int((tb // 2) * (nc - 1) / (tb - 1))] = np.inf                             # a column that bin tb // 2 reads
    x[3, nc - 1] = -np.inf
    x[4, nc - 1] = np.inf
    # (one row at a time: SciPy also interpolates along the axis it does not resize, x[r] * 1 + x[r + 1] * 0, which turns an
    # Inf or NaN of row r + 1 into a NaN of row r.  Not restated: a normalised clip holds no Inf, and a NaN only together
    # with NaN everywhere -- the case below -- unless the caller hands an unfloored +Inf to the C ABI.)
    with np.errstate(invalid="ignore"):
        z = np.concatenate([zoom(x[r:r + 1], (1, tb / nc), order=1)[:, :tb] for r in range(6)])
        got = O.zoom_linear(x, tb)
    assert z.shape == (6, tb) and np.isnan(z[0, :tb - 1]).all() and np.isnan(z[2]).any()
    assert not _bits(z[:, tb - 1]).any()                                           # +0.0, NaN and Inf rows included
    assert not _bits(got[:, tb - 1]).any()
    np.testing.assert_array_equal(got[[0, 1, 5]], z[[0, 1, 5]])                    # the NaN rows and the plain one: every bin
    # beside an Inf SciPy has NaN where the restatement has the Inf (its zero-weight neighbour of the other axis again)
    fin = np.isfinite(z[2:5])
    assert np.array_equal(got[2:5][fin], z[2:5][fin]) and np.isinf(got[2:5][~fin]).all()
    with np.errstate(invalid="ignore"):
        c = oracle_c.normalise_resize(x, tb)                                       # a NaN clip
        ref = zoom((x - x.min()) / (x.max() - x.min() + dt(1e-8)), (1, tb / nc), order=1)[:, :tb]
    assert np.isnan(ref[:, :tb - 1]).all() and not _bits(ref[:, tb - 1]).any()
    np.testing.assert_array_equal(c, ref)
    assert not _bits(c[:, tb - 1]).any()
    assert not ER.latch_loop(c, *ER.tables([0.7, 0.8, 0.9, 0.95], 0.1, dt)).any()  # and its raster is empty


# ---- the latch restatement ---------------------------------------------------------------------------------------------

def test_latch_restatement_matches_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "encoder.npz"))
    names = sorted(k[:-3] for k in g.files if k.endswith("_in") and not k.startswith("gap005"))
    assert len(names) >= 20
    for n in names:
        x = g[n + "_in"]
        on, off = ER.tables(list(g["thresholds"]), float(g["gap"]), x.dtype)
        np.testing.assert_array_equal(ER.latch_loop(x, on, off), g[n + "_out"], err_msg=n)
        np.testing.assert_array_equal(ER.latch_bits(x, on, off), g[n + "_out"], err_msg=n)
    x = g["gap005_float64_in"]
    on, off = ER.tables([0.5, 0.9, 0.3], 0.05, np.float64)
    np.testing.assert_array_equal(ER.latch_loop(x, on, off), g["gap005_float64_out"])
    np.testing.assert_array_equal(ER.latch_bits(x, on, off), g["gap005_float64_out"])


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_latch_forms_agree_and_equal_the_oracles(oracle_c, dt):
    """Loop form = row-parallel form = oracle/ref_numpy = oracle/lsm_oracle.c, positive, zero and NEGATIVE gaps, values equal
    to a bound, NaN rows, 1 to 8 thresholds, 1 to 130 bins."""
    rng = np.random.default_rng(7)
    for n_rows, n_bins, n_thr, gap in ((1, 1, 1, 0.1), (5, 33, 3, 0.0), (65, 100, 8, 0.05), (7, 130, 5, -0.2), (3, 64, 2, -0.05)):
        x = rng.random((n_rows, n_bins)).astype(dt)
        thr = sorted(rng.uniform(0.15, 0.95, n_thr).tolist(), reverse=True)
        on, off = ER.tables(thr, gap, dt)
        x[0, ::3] = on[0]                                  # values EQUAL to a bound: the comparisons are strict
        x[-1, 1::3] = off[-1]
        if n_rows > 2:
            x[1, n_bins // 2] = np.nan
        want = ER.latch_loop(x, on, off)
        np.testing.assert_array_equal(ER.latch_bits(x, on, off), want)
        np.testing.assert_array_equal(O.encode_hysteresis(x, thr, gap), want)
        np.testing.assert_array_equal(oracle_c.encode_hysteresis(x, thr, gap), want)


def test_generators_are_seeded_and_cross_the_thresholds():
    a, b = ER.walk_db(5, 3, 9, 77), ER.walk_db(5, 3, 9, 77)
    assert np.array_equal(a, b) and not np.array_equal(a, ER.walk_db(6, 3, 9, 77))
    assert ER.walk_db(5, 2, 4, 31, np.float32).dtype == np.float32
    s = ER.step_rows(100)
    assert s.min() == 0.0 and s.max() == 1.0 and s.shape == (4 + 5 * 3, 100)
    assert np.array_equal(ER.step_rows(100, np.float32), s.astype(np.float32))


# ---- teeth: wrong encoders the definition must reject on the GPU tests' own inputs --------------------------------------

def _latch_mutant(spec, on, off, ge=False, word=None):
    """`latch_bits` with `>=` / `<=` for the strict comparisons, or with the latch state dropped at every `word`-th bin."""
    out = np.zeros((spec.shape[0], spec.shape[1], len(on)), dtype=np.uint8)
    active = np.zeros((spec.shape[0], len(on)), dtype=bool)
    for j in range(spec.shape[1]):
        x = spec[:, j, None]
        if word and j % word == 0:
            active[:] = False
        up, dn = (x >= on[None, :], x <= off[None, :]) if ge else (x > on[None, :], x < off[None, :])
        active = np.where(active, ~dn, up)
        out[:, j, :] = active
    return out.reshape(spec.shape[0], -1)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_definition_rejects_non_strict_comparisons(oracle_c, dt):
    """Thresholds taken from the normalised values themselves (as the GPU test does): `>=` for `>` changes the raster."""
    db = ER.walk_db(11, 1, 5, 64, dt)[0]
    norm, _ = ER.expected(oracle_c, db, 64, [], [])
    on = np.sort(norm[1, [9, 40]])[::-1].copy()
    off = np.sort(norm[3, [5, 50]])[::-1].copy()
    off = np.minimum(off, on)
    assert (norm[:, :, None] == on).any() and (norm[:, :, None] == off).any()
    want = ER.latch_loop(norm, on, off)
    assert np.array_equal(_latch_mutant(norm, on, off), want)
    assert not np.array_equal(_latch_mutant(norm, on, off, ge=True), want)


def test_definition_rejects_a_latch_not_carried_across_a_word():
    x = ER.step_rows(100)
    on, off = np.array([0.7]), np.array([0.3])
    want = ER.latch_loop(x, on, off)
    got = _latch_mutant(x, on, off, word=32)
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert len(rows) >= 2 and want[8, 32:].all() and not got[8, 32]      # row 8: on at bin 31, held by 0.5 from bin 32 on
    neg = ER.latch_loop(x, np.array([0.3]), np.array([0.7]))             # negative gap: 0.5 flips the latch every bin
    assert np.array_equal(neg[8, 31:37], [1, 0, 1, 0, 1, 0])


@pytest.mark.parametrize("nc,tb,dt", [(105, 100, np.float64), (58, 100, np.float32), (30, 8, np.float64), (8, 26, np.float32),
                                      (32, 31, np.float64)])
def test_definition_rejects_a_resize_without_the_zero_rule(oracle_c, nc, tb, dt):
    """The resize as it was before (x[ncols-1] * w0 in the last bin) against SciPy at the GPU test's overshooting widths:
    the values differ in the last bin only, and the rasters do -- latches that are on in bin tb-2 stay on without the rule."""
    db = ER.plateau_db(nc * tb, 2, 7, nc, dt)
    on, off = ER.tables([0.7, 0.8, 0.9, 0.95], 0.1, dt)
    for b in range(2):
        norm, raster = ER.expected(oracle_c, db[b], tb, on, off)
        fl = ER.floored(db[b])
        full = ((fl - fl.min()) / (dt(fl.max() - fl.min()) + dt(1e-8))).astype(dt)
        zf = (nc - 1) / (tb - 1)
        cc = (tb - 1) * zf
        old = norm.copy()
        old[:, tb - 1] = (full[:, nc - 1].astype(np.float64) * (1.0 - (cc - np.floor(cc)))).astype(dt)
        assert np.array_equal(old[:, :tb - 1], norm[:, :tb - 1]) and not _bits(norm[:, tb - 1]).any()
        assert (old[:, tb - 1] > 0.5).any()
        held = raster.reshape(7, tb, 4)[:, tb - 2, :].any()
        assert held and not raster.reshape(7, tb, 4)[:, tb - 1, :].any()
        assert ER.latch_loop(old, on, off).reshape(7, tb, 4)[:, tb - 1, :].any()
