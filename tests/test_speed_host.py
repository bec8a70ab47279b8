"""Speed perturbation (SPEC.md 1.12): what can be checked without a GPU -- the new public header, its ctypes table and the
library's exports, lsm_speed_lds_bytes (host only), the NumPy restatement (tests/speed_restatement.py) against
`scipy.signal.resample_poly` and its tail of zeros, the designs, the plan and the scripts' flags."""
import ctypes as C
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import speed_restatement as SR  # noqa: E402

NEW_EXPORTS = {"lsm_speed_lds_bytes": 2, "lsm_speed_f32": 12}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("
FACTORS = ["9/10", "11/10", "0.95", "1.05", "0.8", "1.25", "1/2", "2", "0.99", "1.01"]


def _rows(tables):
    """The (n, 5) int32 design rows of a bank: up, down, n_taps, delay, tap_offset."""
    offsets = np.cumsum([0] + [len(t.taps) for t in tables])
    return np.ascontiguousarray([[t.up, t.down, len(t.taps), t.delay, int(o)] for t, o in zip(tables, offsets)], dtype=np.int32)


def _lds_bytes(lib, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    return int(lib.lsm_speed_lds_bytes(C.c_void_p(rows.ctypes.data), len(rows)))


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_two_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_speed.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.SPEED_SYMBOLS == tuple(_lib.SPEED_SIGS) and set(_lib.SPEED_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long)\s+%s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.SPEED_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert (res is _lib.c_int and result == "int") or (res is _lib.C.c_long and result == "long")
        for p, ctype in zip(params, args):                          # a pointer is a void pointer, every scalar an int
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"


def test_the_new_table_is_disjoint_from_the_other_eight_and_the_record_is_59():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
              _lib.MIX_SIGS, _lib.REVERB_SIGS)
    for table in others:
        assert not set(NEW_EXPORTS) & set(table)
    assert len(_lib.EXPORTED_SYMBOLS) == 38                         # include/lsm_hip.h's own table stays as it is
    assert sum(len(t) for t in others) + len(_lib.SPEED_SIGS) == 59


def test_the_library_exports_both_functions_and_the_build_covers_the_new_files():
    from lsm_speech_classifier_amd import _lib, build
    assert "lsm_hip_speed.h" in build.PUBLIC_HEADERS and "speed.hip" in build.SOURCES
    assert len(build.PUBLIC_HEADERS) == 9
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name


def test_lds_bytes_of_a_bank_is_its_largest_table_and_0_for_a_bank_that_would_be_refused():
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    t11, t9, t401 = frontend.speed_design("11/10"), frontend.speed_design("9/10"), frontend.speed_design("401/400")
    assert _lds_bytes(lib, _rows([t11])) == 2000
    assert (t401.up, t401.down) == (400, 401) and _lds_bytes(lib, _rows([t401])) > 65536

    def table_bytes(t):
        return t.up * (-(-len(t.taps) // t.up) | 1) * 8
    bank = [t9, t11, t401, frontend.speed_design("2"), frontend.speed_design("1/2")]
    assert _lds_bytes(lib, _rows(bank)) == max(table_bytes(t) for t in bank) == table_bytes(t401)
    assert _lds_bytes(lib, _rows([t11, t9])) == max(table_bytes(t9), 2000)
    good = _rows([t11])[0].tolist()
    assert _lds_bytes(lib, [good, [10, 10, 232, 0, 0]]) == 0         # up == down
    assert _lds_bytes(lib, [good, [20, 22, 232, 0, 0]]) == 0         # a shared factor
    assert _lds_bytes(lib, [good] * 17) == 0 and _lds_bytes(lib, [good] * 16) == 2000
    assert _lds_bytes(lib, [[10, 11, 0, 0, 0]]) == 0 and _lds_bytes(lib, [[10, 11, 232, 22, 0]]) == 0    # taps, delay
    assert _lds_bytes(lib, [[10, 11, 232, 11, -1]]) == 0 and _lds_bytes(lib, [[0, 11, 232, 0, 0]]) == 0
    assert _lds_bytes(lib, [[1000, 1001, 21022, 0, 0]]) == 0         # 184000 bytes: over a compute unit's LDS
    assert int(lib.lsm_speed_lds_bytes(None, 1)) == 0 and int(lib.lsm_speed_lds_bytes(C.c_void_p(_rows([t11]).ctypes.data), 0)) == 0


# ---- the restatement of SPEC.md 1.12 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS)
def test_the_restatement_against_resample_poly_and_its_tail_of_zeros(factor):
    from scipy.signal import resample_poly
    from lsm_speech_classifier_amd import frontend
    table = frontend.speed_design(factor)
    n_in = 3000
    x = (np.random.default_rng(sum(factor.encode())).standard_normal(n_in) * 0.1).astype(np.float32)
    head, zeros = -(-n_in * table.up // table.down), SR.zero_from(n_in, table)
    assert head < zeros
    y = SR.perturb(x, table, zeros + 64)
    ref = resample_poly(x.astype(np.float64), table.up, table.down)
    assert len(ref) == head and y.dtype == np.float32
    err, bound = np.abs(y[:head].astype(np.float64) - ref).max(), 2.0 ** -23 * np.abs(ref).max()
    print(f"{factor}: up={table.up} down={table.down}: max |y - ref| = {err:.3e} = {err / bound:.2f} of the bound")
    assert err <= bound
    assert not y[zeros:].view(np.uint32).any()                      # the bits of +0.0
    assert y[head:zeros].any()                                      # in between the filter rings out
    # int16 input is the same clip widened by 2^-15
    xi = np.round(x * 8000).astype(np.int16)
    assert SR.perturb(xi, table, 500).tobytes() == SR.perturb(xi.astype(np.float32) * np.float32(2.0 ** -15), table, 500).tobytes()


def test_the_batch_restatement_clamps_rows_and_copies_clips_without_a_design():
    from lsm_speech_classifier_amd import frontend
    tables = [frontend.speed_design("9/10"), frontend.speed_design("11/10")]
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((4, 300)) * 0.1).astype(np.float32)
    x[2, 3], x[2, 4] = np.float32(-0.0), np.float32(np.nan)
    out = SR.perturb_batch(x, tables, [0, 7, -1, -5], 320)
    assert out[0].tobytes() == SR.perturb(x[0], tables[0], 320).tobytes()
    assert out[1].tobytes() == SR.perturb(x[1], tables[1], 320).tobytes()         # clamped to the last row
    assert out[2, :300].tobytes() == x[2].tobytes() and not out[2, 300:].view(np.uint32).any()
    assert out[3, :300].tobytes() == x[3].tobytes()
    assert SR.perturb_batch(x, tables, None, 100).tobytes() == SR.perturb_batch(x, tables, [0] * 4, 100).tobytes()
    assert SR.perturb_batch(x, tables, [-1] * 4, 100).tobytes() == np.ascontiguousarray(x[:, :100]).tobytes()
    xi = np.array([[-32768, 1, 32767]], dtype=np.int16)
    assert SR.perturb_batch(xi, tables, [-1], 4).tolist() == [[-1.0, 2.0 ** -15, 32767 / 32768, 0.0]]


# ---- designs, plan ---------------------------------------------------------------------------------------------------------
def test_speed_design_values_and_refusals():
    from lsm_speech_classifier_amd import frontend
    t = frontend.speed_design("9/10")
    assert (t.up, t.down, len(t.taps), t.delay, t.history) == (10, 9, 209, 12, 20)
    t = frontend.speed_design("11/10")
    assert (t.up, t.down, len(t.taps), t.delay, t.history) == (10, 11, 232, 11, 23)
    ref = frontend.resample_table(17600, 16000)
    for same in (Fraction(11, 10), 1.1, "1.1", np.float64(1.1)):
        again = frontend.speed_design(same)
        assert again[:2] == ref[:2] and again.taps.tobytes() == ref.taps.tobytes() and again[3:] == ref[3:]
    assert frontend.speed_design(2).up == 1 and frontend.speed_design(2).down == 2
    assert frontend.speed_design("1/2").up == 2 and frontend.speed_design(0.5).down == 1
    for one in (1, 1.0, "1", "1.0", Fraction(3, 3)):
        assert frontend.speed_design(one) is None
    with pytest.raises(ValueError, match="184000"):
        frontend.speed_design("1.001")
    with pytest.raises(ValueError, match="integer"):
        frontend.speed_design("4/3")
    for bad in ("0.49", "2.0001", 3, 0, -1, "x", "1/0", None, True, [1.1]):
        with pytest.raises(ValueError):
            frontend.speed_design(bad)
    tables, row_of_choice = frontend.speed_bank(["0.9", 1.0, "1.1"])
    assert [(t.up, t.down) for t in tables] == [(10, 9), (10, 11)] and row_of_choice.tolist() == [0, -1, 1]
    assert row_of_choice.dtype == np.int32
    twentieths = [Fraction(k, 20) for k in range(10, 28) if k != 20]           # 17 designs
    assert len(frontend.speed_bank(twentieths[:16] + [1])[0]) == 16
    for bad in ([], ["0.9", "9/10"], [1, "1.0"], twentieths):
        with pytest.raises(ValueError):
            frontend.speed_bank(bad)


def test_speed_plan_is_deterministic_and_leaves_the_other_plans_alone():
    from lsm_speech_classifier_amd import frontend
    mix_before = frontend.mix_plan(40, 3, 100, (0.0, 20.0), max_shift=10, level_db=(-6.0, 0.0), seed=11)
    rooms_before = frontend.reverb_plan(200, 5, prob=0.7, seed=11)
    a, b = frontend.speed_plan(200, 3, prob=0.7, seed=11), frontend.speed_plan(200, 3, prob=0.7, seed=11)
    assert a.choice.dtype == np.int32 and np.array_equal(a.choice, b.choice)
    rs = np.random.RandomState([11, 2])
    choice = rs.randint(0, 3, size=200)
    u = rs.random_sample(200)
    assert np.array_equal(a.choice, np.where(u >= 0.7, -1, choice))
    assert set(a.choice.tolist()) == {-1, 0, 1, 2}
    assert (frontend.speed_plan(50, 3).choice >= 0).all() and (frontend.speed_plan(50, 3, prob=0.0).choice == -1).all()
    assert not np.array_equal(a.choice, frontend.speed_plan(200, 3, prob=0.7, seed=12).choice)
    assert np.array_equal(a.part(10, 20).choice, a.choice[10:20]) and np.array_equal(a.take([5, 3]).choice, a.choice[[5, 3]])
    assert len(frontend.speed_plan(0, 3).choice) == 0
    # the other plans' draws for the same seed: generators of their own, unchanged by this one
    mix_after = frontend.mix_plan(40, 3, 100, (0.0, 20.0), max_shift=10, level_db=(-6.0, 0.0), seed=11)
    for before, after in zip(mix_before, mix_after):
        assert np.array_equal(before, after)
    ref = np.random.RandomState(11)
    assert np.array_equal(mix_after.rows, ref.randint(0, 3, size=40))
    assert np.array_equal(frontend.reverb_plan(200, 5, prob=0.7, seed=11).rows, rooms_before.rows)
    rs = np.random.RandomState([11, 1])
    rows = rs.randint(0, 5, size=200)
    assert np.array_equal(rooms_before.rows, np.where(rs.random_sample(200) >= 0.7, -1, rows))
    assert not np.array_equal(frontend.speed_plan(200, 5, prob=0.7, seed=11).choice, rooms_before.rows)
    with pytest.raises(ValueError):
        frontend.speed_plan(5, 0)
    with pytest.raises(ValueError):
        frontend.speed_plan(5, 2, prob=1.5)


def test_no_gpu_means_loud_failure_for_the_perturber():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lsm_speech_classifier_amd import _lib, frontend
    with pytest.raises(_lib.LsmHipError):
        frontend.SpeedPerturber(["0.9", "1.1"])
    with pytest.raises(ValueError):                                 # refused on the host, before any device
        frontend.SpeedPerturber([1.0])


# ---- the scripts' flags ----------------------------------------------------------------------------------------------------
def test_speed_flags_parse_and_nothing_without_them():
    import argparse
    import create_dataset as cd
    ap = argparse.ArgumentParser()
    cd.add_augment_flags(ap)
    cd.add_reverb_flags(ap)
    cd.add_speed_flags(ap)
    none = ap.parse_args([])
    assert cd.speed_from_args(none) is None and cd.reverb_from_args(none) is None and cd.augment_from_args(none) is None
    assert none.speed_prob == 1.0
    a = ap.parse_args(["--speed-factors", "0.9,1.0,1.1", "--speed-prob", "0.5", "--augment-seed", "9"])
    pace = cd.speed_from_args(a)
    assert pace == dict(factors=["0.9", "1.0", "1.1"], prob=0.5, seed=9)
    assert cd.augment_from_args(a) is None and cd.reverb_from_args(a) is None
    factors, plan = cd.speeds(pace, 40)
    assert factors == ["0.9", "1.0", "1.1"]
    assert np.array_equal(plan.choice, cd._frontend().speed_plan(40, 3, prob=0.5, seed=9).choice) and (plan.choice == -1).any()
    for bad in (["--speed-factors", "0.9", "--speed-prob", "2"], ["--speed-factors", "0.9,4/3"], ["--speed-factors", "3"],
                ["--speed-factors", "1.0"], ["--speed-factors", "0.9,0.90"], ["--speed-factors", "1.001"]):
        with pytest.raises(SystemExit):
            cd.speed_from_args(ap.parse_args(bad))
    import inspect
    assert inspect.signature(cd.create_dataset).parameters["speed"].default is None


def test_main_forwards_the_speed_flags_to_stage_1_and_nothing_without_them(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert calls[0][1:] == [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, speed_factors="0.9,1.0,1.1", speed_prob=0.5, augment_seed=7)
    assert calls[0][6:] == ["--speed-factors", "0.9,1.0,1.1", "--speed-prob", "0.5", "--augment-seed", "7"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, rir_dir="synthetic", speed_factors="1.1")
    assert calls[0][6:] == ["--rir-dir", "synthetic", "--rir-prob", "1.0", "--rir-max-ms", "500.0", "--augment-seed", "42",
                            "--speed-factors", "1.1", "--speed-prob", "1.0"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, speed_factors="0.9,1.1")
    code = calls[0][2]
    assert "'speed_factors': '0.9,1.1'" in code and "'speed_prob': 1.0" in code and "speed=speed" in code
    with pytest.raises(TypeError):
        pipeline.run_pipeline(128, "gammatone", "original", 0.6, speed_seed=1)
