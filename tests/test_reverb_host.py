"""Reverberation (SPEC.md 1.11): what can be checked without a GPU -- the new public header, its ctypes table and the
library's exports, the NumPy restatement of the arithmetic (tests/reverb_restatement.py) against `np.convolve` and against
itself cut into pushes, the ground of the fused multiply-add clause, the plans, the synthetic bank and the scripts' flags."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reverb_restatement as RR  # noqa: E402

NEW_EXPORTS = {"lsm_reverb_state_bytes": 1, "lsm_reverb_f32": 11, "lsm_reverb_stream_f32": 13}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def _same(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def _decaying(K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(K) * np.exp(-np.arange(K) / max(1.0, K / 5.0))).astype(np.float32)


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_three_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_reverb.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.REVERB_SYMBOLS == tuple(_lib.REVERB_SIGS) and set(_lib.REVERB_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long)\s+%s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.REVERB_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert (res is _lib.c_int and result == "int") or (res is _lib.C.c_long and result == "long")
        for p, ctype in zip(params, args):                          # a pointer is a void pointer, every scalar an int
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"


def test_the_new_table_is_disjoint_from_all_the_others_and_the_record_is_57():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
              _lib.MIX_SIGS)
    for table in others:
        assert not set(NEW_EXPORTS) & set(table)
    assert len(_lib.EXPORTED_SYMBOLS) == 38                         # include/lsm_hip.h's own table stays as it is
    assert sum(len(t) for t in others) + len(_lib.REVERB_SIGS) == 57


def test_the_library_exports_every_function_the_header_declares_and_the_build_covers_the_new_files():
    from lsm_speech_classifier_amd import _lib, build
    assert "lsm_hip_reverb.h" in build.PUBLIC_HEADERS and "reverb.hip" in build.SOURCES and "reverb_body.h" in build.HEADERS
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert lib.lsm_reverb_state_bytes(1) == 16 and lib.lsm_reverb_state_bytes(700) == 2800 and lib.lsm_reverb_state_bytes(0) == 0


# ---- the restatement of SPEC.md 1.11 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 63, 700, 1500, 8000])
def test_anchor_1_the_restatement_against_np_convolve_within_one_float32_rounding(K):
    n = 4096
    x = (np.random.default_rng(K).standard_normal(n) * 0.1).astype(np.float32)
    h = _decaying(K, 1000 + K)
    y = RR.convolve(x, h)
    ref = np.convolve(x.astype(np.float64), h.astype(np.float64))[:n]
    err, bound = np.abs(y.astype(np.float64) - ref).max(), 2.0 ** -23 * np.abs(ref).max()
    print(f"K={K}: max |y - ref| = {err:.3e} = {err / bound:.2f} of the bound")
    assert y.dtype == np.float32 and err <= bound


def test_anchor_2_integer_values_equal_np_convolve_exactly():
    rng = np.random.default_rng(2)
    n, K = 3000, 257
    x = rng.integers(-1000, 1001, n).astype(np.float32)
    h = rng.integers(-500, 501, K).astype(np.float32)
    xi, hi = x.astype(np.int64), h.astype(np.int64)
    want = np.convolve(xi, hi)
    # the inputs' own property: every partial sum in the specified order is an integer below 2^24 (exact in float32 too)
    ext = np.concatenate([np.zeros(K - 1, dtype=np.int64), xi, np.zeros(K, dtype=np.int64)])
    part, peak = np.zeros(n + K - 1, dtype=np.int64), 0
    for k in range(K):
        part = part + hi[k] * ext[K - 1 - k:K - 1 - k + n + K - 1]
        peak = max(peak, int(np.abs(part).max()))
    assert np.array_equal(part, want) and peak < 2 ** 24
    full = RR.convolve(x, h, n + K - 1)
    assert np.array_equal(full.astype(np.int64), want) and np.array_equal(full, want.astype(np.float32))
    assert np.array_equal(RR.convolve(x, h), full[:n])


def test_products_of_float32_pairs_are_exact_in_float64():
    """The ground of the FMA clause: (double)a * (double)b is the exact product, so fma(a, b, acc) == acc + a * b."""
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(3000) * 10.0 ** rng.integers(-20, 18, 3000)).astype(np.float32)
    b = (rng.standard_normal(3000) * 10.0 ** rng.integers(-20, 18, 3000)).astype(np.float32)
    a[:4] = np.array([np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1.4e-45, -np.finfo(np.float32).max], dtype=np.float32)
    b[:4] = np.array([np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1.4e-45, np.finfo(np.float32).max], dtype=np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)
    assert np.isfinite(prod).all()
    for u, v, p in zip(a, b, prod):
        assert Fraction(float(u)) * Fraction(float(v)) == Fraction(float(p))


def test_streamed_restatement_cut_anywhere_equals_the_uncut_run_and_the_batch_form():
    rng = np.random.default_rng(4)
    n, K = 3000, 300
    bank = np.stack([_decaying(K, 41), _decaying(K, 42)])
    lengths = np.array([K, 120], dtype=np.int32)
    x = (rng.standard_normal(n) * 0.1).astype(np.float32)
    for row in (0, 1):
        uncut, state = RR.stream_cut(x, bank, [n], lengths, row)
        assert _same(uncut, RR.reverb(x[None, :], bank, lengths, [row])[0])
        assert _same(state, x[n - (K - 1):])
        for trial in range(4):
            cuts, left = [], n
            while left:
                c = min(left, int(rng.choice([0, 1, 5, K - 2, K - 1, K, K + 7, 1000])))
                cuts.append(c)
                left -= c
            got, st = RR.stream_cut(x, bank, cuts, lengths, row)
            assert _same(got, uncut) and _same(st, state), (row, cuts)
    got, st = RR.stream_cut(x, bank, [0, 1, 0, 2, n - 3], lengths, 1)
    assert _same(got, RR.stream_cut(x, bank, [n], lengths, 1)[0])


def test_a_row_changed_between_pushes_follows_the_history_rule_and_a_dry_row_keeps_minus_zero():
    rng = np.random.default_rng(5)
    K = 50
    bank = np.stack([_decaying(K, 51), _decaying(K, 52)])
    lengths = np.array([K, 10], dtype=np.int32)
    x = (rng.standard_normal(400) * 0.1).astype(np.float32)
    x[3] = np.float32(-0.0)
    got, state = RR.stream_cut(x, bank, [150, 250], lengths, [1, 0])
    # the second push, row 0 of 50 taps, sees the 49 samples in front of it although row 1 needed only 9
    want_tail = RR.convolve(x[150:], bank[0], history=x[:150])
    assert _same(got[150:], want_tail) and _same(got[:150], RR.convolve(x[:150], bank[1, :10]))
    assert _same(got[150:], RR.convolve(x, bank[0])[150:])
    dry, st = RR.stream_cut(x, bank, [100, 300], lengths, [-1, -1])
    assert _same(dry, x) and np.signbit(dry[3]) and _same(st, x[-(K - 1):])
    batch = RR.reverb(x[None, :], bank, lengths, [-1], n_out=405)
    assert _same(batch[0, :400], x) and not batch[0, 400:].any() and not np.signbit(batch[0, 400:]).any()
    assert _same(RR.reverb(x[None, :], bank, lengths, [7]), RR.reverb(x[None, :], bank, lengths, [1]))      # clamped
    nan = x.copy()
    nan[200] = np.nan
    assert np.isnan(RR.reverb(nan[None, :], bank, lengths, [1])[0]).nonzero()[0].tolist() == list(range(200, 210))


# ---- plans, the synthetic bank --------------------------------------------------------------------------------------------
def test_reverb_plan_is_deterministic_and_leaves_mix_plan_alone():
    from lsm_speech_classifier_amd import frontend
    a, b = frontend.reverb_plan(200, 5, prob=0.7, seed=11), frontend.reverb_plan(200, 5, prob=0.7, seed=11)
    assert a.rows.dtype == np.int32 and np.array_equal(a.rows, b.rows)
    rs = np.random.RandomState([11, 1])
    rows = rs.randint(0, 5, size=200)
    u = rs.random_sample(200)
    assert np.array_equal(a.rows, np.where(u >= 0.7, -1, rows))
    assert (a.rows == -1).any() and set(a.rows.tolist()) == {-1, 0, 1, 2, 3, 4}
    assert (frontend.reverb_plan(50, 3).rows >= 0).all() and (frontend.reverb_plan(50, 3, prob=0.0).rows == -1).all()
    assert not np.array_equal(a.rows, frontend.reverb_plan(200, 5, prob=0.7, seed=12).rows)
    assert np.array_equal(a.part(10, 20).rows, a.rows[10:20]) and np.array_equal(a.take([5, 3]).rows, a.rows[[5, 3]])
    # the first 50 clips of a longer listing are not the plan of a listing of 50: a shard takes its part of the whole plan
    # mix_plan's draws for the same seed: what np.random.RandomState(seed) gives, as before
    m = frontend.mix_plan(40, 3, 100, (0.0, 20.0), max_shift=10, level_db=(-6.0, 0.0), seed=11)
    ref = np.random.RandomState(11)
    assert np.array_equal(m.rows, ref.randint(0, 3, size=40)) and np.array_equal(m.offsets, ref.randint(0, 100, size=40))
    assert np.array_equal(m.shift, ref.randint(-10, 11, size=40))
    assert np.array_equal(m.snr_db, 0.0 + 20.0 * ref.random_sample(40))
    with pytest.raises(ValueError):
        frontend.reverb_plan(5, 0)
    with pytest.raises(ValueError):
        frontend.reverb_plan(5, 2, prob=1.5)


def test_room_responses_are_deterministic():
    from lsm_speech_classifier_amd import synth
    bank, lengths = synth.room_responses(4)
    again, _ = synth.room_responses(4)
    assert bank.dtype == np.float32 and lengths.dtype == np.int32 and bank.tobytes() == again.tobytes()
    assert lengths.tolist() == [int(0.2 * 16000), int(0.4 * 16000), int((0.2 + 0.6 * 2 / 3) * 16000), int(0.8 * 16000)]
    assert bank.shape == (4, 12800) and (bank[:, 0] == 1).all()
    for r, n in enumerate(lengths):
        assert not bank[r, n:].any() and bank[r, n - 1] != 0
    # the restated recipe
    rs = np.random.RandomState(1234)
    g = rs.standard_normal(3200)
    h = 0.05 * g * 10.0 ** (-3.0 * np.arange(3200) / 3200.0)
    h[0] = 1.0
    assert bank[0, :3200].tobytes() == h.astype(np.float32).tobytes()
    early, late = np.abs(bank[3, 1:641]).mean(), np.abs(bank[3, -640:]).mean()
    assert 50.0 < 20 * np.log10(early / late) < 62.0                # close to -60 dB at the row's end
    one, n1 = synth.room_responses(1, rt60=0.3, seed=5)
    assert one.shape == (1, 4800) and n1.tolist() == [4800]
    assert synth.room_responses(2, seed=1)[0].tobytes() != synth.room_responses(2, seed=2)[0].tobytes()


def test_checked_bank_refusals_before_any_device():
    from lsm_speech_classifier_amd import frontend
    ok = np.zeros((2, 10), dtype=np.float32)
    for bad in (np.zeros((2, 10)), np.zeros((2, 0), dtype=np.float32), np.zeros((1, 16385), dtype=np.float32),
                np.zeros((2, 2, 2), dtype=np.float32)):
        with pytest.raises(ValueError):
            frontend.checked_rir_bank(bad)
    for bad in ([1, 11], [0, 5], [1, 2, 3]):
        with pytest.raises(ValueError):
            frontend.checked_rir_bank(ok, bad)
    bank, lengths = frontend.checked_rir_bank(ok[0], [10])
    assert tuple(bank.shape) == (1, 10) and lengths.tolist() == [10]


def test_no_gpu_means_loud_failure_for_the_reverberator():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lsm_speech_classifier_amd import _lib, frontend
    with pytest.raises(_lib.LsmHipError):
        frontend.Reverberator(np.ones((2, 100), dtype=np.float32))


# ---- the scripts' flags ----------------------------------------------------------------------------------------------------
def test_main_forwards_the_reverb_flags_to_stage_1_and_nothing_without_them(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert calls[0][1:] == [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, rir_dir="synthetic", rir_prob=0.5, augment_seed=7)
    assert calls[0][6:] == ["--rir-dir", "synthetic", "--rir-prob", "0.5", "--rir-max-ms", "500.0", "--augment-seed", "7"]
    assert calls[1][1:] == [os.path.join(ROOT, "extract_lsm_features.py"), "--feature-set", "original", "--multiplier", "0.6"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, noise_dir="synthetic", rir_dir="rooms", rir_max_ms=250.0)
    assert calls[0][6:] == ["--noise-dir", "synthetic", "--augment-seed", "42", "--rir-dir", "rooms", "--rir-prob", "1.0",
                            "--rir-max-ms", "250.0"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, rir_dir="synthetic")
    code = calls[0][2]
    assert "'rir_dir': 'synthetic'" in code and "'rir_prob': 1.0" in code and "reverb=reverb" in code
    with pytest.raises(TypeError):
        pipeline.run_pipeline(128, "gammatone", "original", 0.6, rir_seed=1)


def test_reverb_flags_parse_and_load_rir_bank(tmp_path):
    import argparse
    import create_dataset as cd
    from scipy.io import wavfile
    ap = argparse.ArgumentParser()
    cd.add_augment_flags(ap)
    cd.add_reverb_flags(ap)
    none = ap.parse_args([])
    assert cd.reverb_from_args(none) is None and cd.augment_from_args(none) is None
    assert (none.rir_prob, none.rir_max_ms) == (1.0, 500.0)
    a = ap.parse_args(["--rir-dir", "synthetic", "--rir-prob", "0.25", "--rir-max-ms", "100", "--augment-seed", "9"])
    room = cd.reverb_from_args(a)
    assert room == dict(rir_dir="synthetic", prob=0.25, max_ms=100.0, seed=9) and cd.augment_from_args(a) is None
    bank, lengths, plan = cd.reverberation(room, 40)
    assert bank.shape == (cd.SYNTHETIC_RIR_ROWS, 1600) and lengths.tolist() == [1600] * 4 and (bank[:, 0] == 1).all()
    assert np.array_equal(plan.rows, cd._frontend().reverb_plan(40, 4, prob=0.25, seed=9).rows) and (plan.rows == -1).any()
    full, full_lengths = cd.load_rir_bank("synthetic")
    assert full.shape == (4, 8000) and full_lengths.tolist() == [3200, 6400, 8000, 8000]
    for bad in (["--rir-dir", "x", "--rir-prob", "2"], ["--rir-dir", "x", "--rir-max-ms", "0"]):
        with pytest.raises(SystemExit):
            cd.reverb_from_args(ap.parse_args(bad))
    with pytest.raises(ValueError, match="16384"):
        cd.load_rir_bank("synthetic", max_ms=2000.0)
    # two wav files: a delayed, negative direct path with trailing zeros at 16 kHz, and one at 8 kHz
    h = np.zeros(500, dtype=np.int16)
    h[40], h[41], h[100], h[299] = -20000, 5000, -2500, 1250
    wavfile.write(str(tmp_path / "b_room.wav"), 16000, h)
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(300) * 2000 * np.exp(-np.arange(300) / 60.0)).astype(np.int16)
    g[0] = 30000
    wavfile.write(str(tmp_path / "a_hall.wav"), 8000, g)
    wavfile.write(str(tmp_path / "c_silent.wav"), 16000, np.zeros(100, dtype=np.int16))
    bank, lengths = cd.load_rir_bank(str(tmp_path), max_ms=10.0)     # at most 160 taps
    assert bank.shape[0] == 2 and bank.dtype == np.float32 and lengths.dtype == np.int32 and (bank[:, 0] == 1).all()
    assert lengths[1] == 61 and bank.shape[1] == max(lengths) <= 160
    assert bank[1, 1] == np.float32(-0.25) and bank[1, 60] == np.float32(0.125) and not bank[1, 61:].any()
    assert np.abs(bank[0]).max() == 1.0 and lengths[0] <= 160
    bank, lengths = cd.load_rir_bank(str(tmp_path), max_ms=500.0)
    assert lengths[1] == 260 and bank[1, 259] == np.float32(-0.0625)
    with pytest.raises(ValueError, match="no readable wav"):
        cd.load_rir_bank(str(tmp_path / "nothing"))
