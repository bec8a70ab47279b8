"""Adaptive normalisation range (SPEC.md 1.9): what can be checked without a GPU -- the new public header, its ctypes table
and the library's exports, the state block's size, and the NumPy restatement of the arithmetic
(tests/adaptive_restatement.py) against the pinned per-clip code of SPEC.md 1.2 and against itself cut into pushes."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adaptive_restatement as A  # noqa: E402

NEW_EXPORTS = {"lsm_adaptive_state_bytes": 3, "lsm_adaptive_encode_f64": 16, "lsm_adaptive_encode_f32": 16}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def _db(dtype, seed, shape=(7, 40), span=120.0):
    """Random dB values spanning more than the 80 dB floor."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-span, 0.0, size=shape)).astype(dtype)


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_three_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_adaptive.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.ADAPTIVE_SYMBOLS == tuple(_lib.ADAPTIVE_SIGS) and set(_lib.ADAPTIVE_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long)\s+%s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.ADAPTIVE_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is (_lib.c_int if result == "int" else _lib.C.c_long)
        for p, ctype in zip(params, args):                          # a pointer is a void pointer, every scalar an int
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    for name, elem in (("lsm_adaptive_encode_f64", "double"), ("lsm_adaptive_encode_f32", "float")):
        proto = " ".join(re.search(r"int\s+%s\((.*?)\);" % name, header, re.S).group(1).split())
        assert proto.startswith(f"const {elem} *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols")
        assert "const void *state_in, void *state_out, uint8_t *raster_out" in proto
        assert f"{elem} *lo_out, {elem} *hi_out, void *stream" in proto


def test_the_new_table_is_disjoint_from_all_the_others():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS)
    for table in others:
        assert not set(NEW_EXPORTS) & set(table)
    assert len(_lib.EXPORTED_SYMBOLS) == 38                         # include/lsm_hip.h's own table stays as it is
    assert sum(len(t) for t in others) + len(_lib.ADAPTIVE_SIGS) == 51


def test_the_library_exports_every_function_the_header_declares():
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_adaptive.h")).read()
    declared = set(re.findall(_DECLARED, header, re.M))
    assert declared == set(NEW_EXPORTS)
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in lsm_hip_adaptive.h but not exported"
    blob = open(build.lib_path(), "rb").read()
    for name in declared:
        assert name.encode() + b"\0" in blob


def test_the_build_identity_covers_the_new_header_and_source(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_adaptive.h" in build.PUBLIC_HEADERS and "adaptive_stream.hip" in build.SOURCES
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    with open(inc / "lsm_hip_adaptive.h", "a") as f:
        f.write("\n/* changed */\n")
    assert build.source_id(str(inc)) != build.source_id()


def test_state_bytes():
    from lsm_speech_classifier_amd import _lib
    fn = _lib.load().lsm_adaptive_state_bytes
    for elem in (4, 8):
        sizes = {(F, L): fn(F, L, elem) for F in (1, 2, 64, 65, 130) for L in (1, 2, 7, 100, 4096)}
        for (F, L), nbytes in sizes.items():
            assert nbytes > 0 and nbytes % 16 == 0, (F, L, elem)
            # the cmin and cmax of L - 1 carried columns, a latch word per filter, the count
            assert nbytes >= 2 * (L - 1) * elem + 4 * F + 4, (F, L, elem)
        assert sizes[(130, 100)] > sizes[(65, 100)] > sizes[(2, 100)]
        assert sizes[(64, 4096)] > sizes[(64, 100)] > sizes[(64, 7)] > sizes[(64, 1)]
        assert fn(0, 100, elem) == 0 and fn(-3, 100, elem) == 0
        assert fn(64, 0, elem) == 0 and fn(64, 4097, elem) == 0 and fn(64, -1, elem) == 0
    assert fn(64, 100, 8) > fn(64, 100, 4)
    for elem in (0, 2, 16, -8):
        assert fn(64, 100, elem) == 0


# ---- the restatement of SPEC.md 1.9 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_anchors_to_the_pinned_per_clip_code(dtype):
    """A stream that has held at most L columns is normalised like the reference's clip of those columns: with L = 64 the
    last of 40 columns sees the whole array, floored 80 dB below its maximum as create_dataset.py:60 does."""
    from oracle import ref_numpy
    for seed in range(6):
        db = _db(dtype, seed)
        assert db.max() - db.min() > 80
        norm, lo, hi = A.adaptive(db, 64)
        assert norm.dtype == dtype and lo.dtype == dtype and hi.dtype == dtype
        want = ref_numpy.normalise_resize(np.maximum(db, db.max() - 80), time_bins=40)
        assert want.dtype == dtype and want.shape == norm.shape
        assert norm[:, -1].tobytes() == want[:, -1].tobytes(), f"seed {seed}"
        assert hi[-1] == db.max() and lo[-1] == db.max() - dtype(80)
        # and every earlier column is the pinned code on the columns up to it
        for c in (0, 1, 17):
            part = db[:, :c + 1]
            want_c = ref_numpy.normalise_resize(np.maximum(part, part.max() - 80), time_bins=c + 1) if c else None
            if want_c is not None:
                assert norm[:, c].tobytes() == want_c[:, c].tobytes(), f"seed {seed}, column {c}"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_window_flat_rule_and_nans(dtype):
    db = _db(dtype, 11, shape=(5, 30), span=60.0)
    db[:, 10:20] = dtype(-33.5)                                     # ten identical columns, constant across filters
    db[2, 4] = np.nan
    db[:, 25] = np.nan                                              # a column with no value
    L = 7
    norm, lo, hi = A.adaptive(db, L)
    for c in range(30):
        win = db[:, max(0, c - L + 1):c + 1]
        if np.isnan(win).all():
            continue
        assert hi[c] == np.nanmax(win) and lo[c] == max(np.nanmin(win), np.nanmax(win) - dtype(80)), c
    assert not norm[:, 16:20].any() and (hi[16:20] == lo[16:20]).all()      # windows inside the flat stretch
    assert norm[:, 15].any()                                        # column 9 is still in that window
    assert np.isnan(norm[2, 4]) and not np.isnan(norm[2, 5]) and np.isnan(norm[:, 25]).all()
    assert hi[25] == np.nanmax(db[:, 19:25]) and np.isfinite(norm[:, 26]).all()
    # L = 1: a column alone; the all-NaN column has no range and is flat
    norm1, lo1, hi1 = A.adaptive(db, 1)
    assert hi1[25] == -np.inf and lo1[25] == np.inf and not norm1[:, 25].any()
    assert not norm1[:, 10:20].any()
    finite = ~np.isnan(norm)
    assert (norm[finite] >= 0).all() and (norm[finite] <= 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("L", [1, 2, 7, 100])
def test_restatement_of_a_cut_run_equals_the_uncut_run(dtype, L):
    db = _db(dtype, 5, shape=(6, 60))
    db[1, 7] = np.nan
    norm, lo, hi = A.adaptive(db, L)
    for cuts in ([60], [1] * 60, [0, 3, 37, 20], [59, 1, 0]):
        n2, lo2, hi2, (cmin, cmax) = A.adaptive_cut(db, L, cuts)
        assert n2.tobytes() == norm.tobytes() and lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes(), cuts
        keep = min(L - 1, 60)
        want_min, want_max = A.column_extrema(db[:, 60 - keep:])
        assert cmin.tobytes() == want_min.tobytes() and cmax.tobytes() == want_max.tobytes()
