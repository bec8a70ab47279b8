"""Noise mixer (SPEC.md 1.10): what can be checked without a GPU -- the new public header, its ctypes table and the library's
exports, the NumPy restatement of the arithmetic (tests/mix_restatement.py) against plain NumPy and against itself cut into
pushes, the corruption plan, and the refusals Python makes before anything touches a device."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mix_restatement as M  # noqa: E402

NEW_EXPORTS = {"lsm_mix_power_f32": 5, "lsm_mix_f32": 15, "lsm_mix_stream_f32": 14}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def wide_spread(n, seed=7):
    """float32 samples over some 60 binary orders of magnitude: the order of a float64 sum of their squares shows."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, size=n))).astype(np.float32)


def _clips(B, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, n)) * 0.1).astype(np.float32)


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_three_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_mix.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.MIX_SYMBOLS == tuple(_lib.MIX_SIGS) and set(_lib.MIX_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long)\s+%s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.MIX_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is _lib.c_int and result == "int"
        for p, ctype in zip(params, args):                          # a pointer is a void pointer, every scalar an int
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    proto = " ".join(re.search(r"int\s+lsm_mix_f32\((.*?)\);", header, re.S).group(1).split())
    assert ("const int32_t *noise_row, const int32_t *noise_offset, const int32_t *shift, const float *scale, "
            "const double *ratio, float *out, double *gain_out, double *power_out, void *stream") in proto


def test_the_new_table_is_disjoint_from_all_the_others():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS)
    for table in others:
        assert not set(NEW_EXPORTS) & set(table)
    assert len(_lib.EXPORTED_SYMBOLS) == 38                         # include/lsm_hip.h's own table stays as it is
    assert sum(len(t) for t in others) + len(_lib.MIX_SIGS) == 54


def test_the_library_exports_every_function_the_header_declares():
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_mix.h")).read()
    declared = set(re.findall(_DECLARED, header, re.M))
    assert declared == set(NEW_EXPORTS)
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in lsm_hip_mix.h but not exported"
    blob = open(build.lib_path(), "rb").read()
    for name in declared:
        assert name.encode() + b"\0" in blob


def test_the_build_identity_covers_the_three_new_files(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_mix.h" in build.PUBLIC_HEADERS and "mix.hip" in build.SOURCES and "mix_body.h" in build.HEADERS
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    with open(inc / "lsm_hip_mix.h", "a") as f:
        f.write("x")
    assert build.source_id(str(inc)) != build.source_id()


# ---- the restatement of SPEC.md 1.10 ---------------------------------------------------------------------------------------
def test_ratio_zero_is_the_scaled_shifted_clip_bit_for_bit():
    n = 1000
    audio, noise = _clips(1, n, 1), _clips(2, 300, 2)
    for shift in (-n, -1, 0, 1, n - 1, n, -n - 5, n + 9):
        for scale in (1.0, 2.0 ** -7, 0.3):
            y, g, _ = M.mix(audio, noise, 0.0, shift=shift, scale=scale)
            s = int(np.clip(shift, -n, n))
            want = np.roll(audio[0].astype(np.float64) * np.float64(np.float32(scale)), s)
            if s >= 0:
                want[:s] = 0.0                                      # np.roll wraps; the mixer fills with zeros
            else:
                want[n + s:] = 0.0
            assert y[0].tobytes() == want.astype(np.float32).tobytes(), (shift, scale)
            assert g[0] == 0.0


def test_the_noise_row_wraps_and_offsets_reduce_modulo_its_length():
    n, L = 1000, 37                                                 # L < n: the row wraps 27 times
    audio, noise = _clips(1, n, 3), _clips(3, L, 4)
    v = M.noise_rows(noise, [1], [5], n)
    assert v[0].tobytes() == np.resize(np.roll(noise[1], -5), n).astype(np.float64).tobytes()
    base = M.mix(audio, noise, 1.0, rows=1, offsets=5)
    for off in (5 - L, 5 + L, 5 - 40 * L, 5 + 1000 * L):            # negative and over-long offsets
        other = M.mix(audio, noise, 1.0, rows=1, offsets=off)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, other)), off
    # rows and shifts outside their range are clamped
    for row, clamped in ((-4, 0), (3, 2), (10 ** 6, 2)):
        a, b = M.mix(audio, noise, 1.0, rows=row), M.mix(audio, noise, 1.0, rows=clamped)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    a, b = M.mix(audio, noise, 1.0, shift=n + 100), M.mix(audio, noise, 1.0, shift=n)
    assert a[0].tobytes() == b[0].tobytes() and not a[0].any() and a[1][0] == 0.0     # nothing left of the clip: silence


def test_a_nan_poisons_only_its_own_clip_and_a_nan_bank_never_a_clean_clip():
    audio, noise = _clips(3, 257, 5), _clips(2, 100, 6)
    clean = M.mix(audio, noise, [1.0, 0.1, 0.0], rows=[0, 1, 0])
    audio2 = audio.copy()
    audio2[1, 40] = np.nan
    y, g, P = M.mix(audio2, noise, [1.0, 0.1, 0.0], rows=[0, 1, 0])
    assert np.isnan(y[1]).all() and np.isnan(g[1]) and np.isnan(P[1, 0])
    assert y[0].tobytes() == clean[0][0].tobytes() and y[2].tobytes() == clean[0][2].tobytes()
    noise2 = noise.copy()
    noise2[0, 3] = np.nan
    y, g, P = M.mix(audio, noise2, [1.0, 0.1, 0.0], rows=[0, 1, 0])
    # a NaN row has no power to scale by: !(Pv > 0), so even the clip that asked for noise stays clean
    assert y[0].tobytes() == audio[0].tobytes() and g[0] == 0.0 and np.isnan(P[0, 1])
    assert y[1].tobytes() == clean[0][1].tobytes()                  # another row
    assert y[2].tobytes() == audio[2].tobytes() and g[2] == 0.0     # ratio 0 on the NaN row: clean, bit for bit


def test_anchor_to_plain_numpy_the_achieved_snr_and_the_naive_gain():
    rng = np.random.default_rng(11)
    worst = 0.0
    for case in range(200):
        n = int(rng.integers(1, 3000))
        L = int(rng.integers(1, 4000))
        audio = (rng.standard_normal((1, n)) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32)
        noise = (rng.standard_normal((1, L)) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32)
        snr = float(rng.uniform(-10, 40))
        off, scale = int(rng.integers(0, L)), np.float32(rng.uniform(0.1, 2.0))
        y, g, P = M.mix(audio, noise, 10.0 ** (-snr / 10.0), offsets=off, scale=scale)
        x = np.float64(scale) * audio[0].astype(np.float64)
        v = np.resize(np.roll(noise[0], -off), n).astype(np.float64)
        if not np.sum(v * v) > 0:
            continue
        achieved = 10.0 * np.log10(np.sum(x * x) / np.sum((g[0] * v) ** 2))
        worst = max(worst, abs(achieved - snr))
        assert abs(achieved - snr) <= 1e-9, (case, achieved, snr)
        g_naive = np.sqrt(np.sum(x * x) * 10.0 ** (-snr / 10.0) / np.sum(v * v))
        naive = (x + g_naive * v).astype(np.float32)
        assert np.abs(y[0].astype(np.float64) - naive.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(y[0]).max(), case
    print(f"worst distance from the requested SNR over 200 cases: {worst:.3g} dB")


def test_the_power_order_can_be_told_apart_from_numpys():
    u = wide_spread(16000)
    ours = M.power(u)
    pairwise = np.sum(u.astype(np.float64) ** 2)
    assert np.isfinite(ours) and ours.tobytes() != pairwise.tobytes()
    assert abs(ours - pairwise) <= 1e-12 * pairwise
    # and the order is the stated one: lane by lane, then the tree
    p = np.zeros(256)
    sq = u.astype(np.float64) ** 2
    for k in range(0, len(u), 256):
        part = sq[k:k + 256]
        p[:len(part)] = p[:len(part)] + part
    s = 128
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    assert p[0].tobytes() == ours.tobytes()
    assert M.power(u[:1]) == sq[0]
    assert M.power(u[:257]).tobytes() == _tree(np.concatenate([[sq[0] + sq[256]], sq[1:256]])).tobytes()


def _tree(p):
    p = np.array(p, dtype=np.float64)
    s = len(p) // 2
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def test_streamed_restatement_of_a_cut_run_equals_the_uncut_run():
    n, L = 100, 41                                                  # L smaller than one push
    rng = np.random.default_rng(13)
    x = (rng.standard_normal(n) * 0.1).astype(np.float32)
    noise = _clips(2, L, 14)
    for gain in (0.0, 0.37):
        whole, end = M.stream(x, noise, gain, row=1, scale=0.3, pos=L - 1)
        assert end == (L - 1 + n) % L
        for cuts in ([n], [1] * n, [0, 3, 37, 60], [n - 1, 1, 0]):
            y, pos = M.stream_cut(x, noise, gain, cuts, row=1, scale=0.3, pos=L - 1)
            assert y.tobytes() == whole.tobytes() and pos == end, (gain, cuts)
    clean, _ = M.stream(x, noise, 0.0, scale=0.3)
    assert clean.tobytes() == (np.float64(np.float32(0.3)) * x.astype(np.float64)).astype(np.float32).tobytes()
    # the streamed form with the batch form's gain is the batch form without a shift
    y, g, _ = M.mix(x[None, :], noise, 0.1, rows=1, offsets=7, scale=0.3)
    ys, _ = M.stream(x, noise, g[0], row=1, scale=0.3, pos=7)
    assert ys.tobytes() == y[0].tobytes()


# ---- the plan and Python's refusals ----------------------------------------------------------------------------------------
def test_mix_plan_is_seeded_and_a_shard_takes_its_slice():
    from lsm_speech_classifier_amd import frontend
    kw = dict(n_noise_rows=6, noise_len=960000, snr_db=(0.0, 20.0), max_shift=1600, level_db=(-12.0, 0.0))
    whole = frontend.mix_plan(101, seed=5, **kw)
    again = frontend.mix_plan(101, seed=5, **kw)
    other = frontend.mix_plan(101, seed=6, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(whole, other))
    assert [a.dtype for a in whole] == [np.float64, np.int32, np.int32, np.int32, np.float32]
    assert all(len(a) == 101 for a in whole)
    assert (whole.snr_db >= 0).all() and (whole.snr_db <= 20).all() and len(set(whole.snr_db)) > 50
    assert (np.abs(whole.shift) <= 1600).all() and whole.shift.min() < 0 < whole.shift.max()
    assert (whole.rows >= 0).all() and (whole.rows < 6).all() and (whole.offsets >= 0).all() and (whole.offsets < 960000).all()
    assert (whole.scale <= 1).all() and (whole.scale >= np.float32(10 ** (-12 / 20))).all()
    for ranks in (2, 3):
        bounds = [101 * r // ranks for r in range(ranks + 1)]
        parts = [whole.part(lo, hi) for lo, hi in zip(bounds, bounds[1:])]
        for i, name in enumerate(whole._fields):
            assert np.concatenate([p[i] for p in parts]).tobytes() == whole[i].tobytes(), name
    # scalar forms: constants, and no other array moves
    flat = frontend.mix_plan(101, 6, 960000, 10.0, 0, 0.0, seed=5)
    assert (flat.snr_db == 10.0).all() and not flat.shift.any() and (flat.scale == 1).all()
    assert flat.rows.tobytes() == whole.rows.tobytes() and flat.offsets.tobytes() == whole.offsets.tobytes()
    assert np.isinf(frontend.mix_plan(4, 1, 10, np.inf).snr_db).all()
    assert len(frontend.mix_plan(0, 1, 10, 5.0).rows) == 0
    for bad in (dict(snr_db=np.nan), dict(snr_db=-np.inf), dict(snr_db=(5.0, 1.0)), dict(snr_db=(1.0, 2.0, 3.0))):
        with pytest.raises(ValueError):
            frontend.mix_plan(4, 1, 10, **bad)
    with pytest.raises(ValueError):
        frontend.mix_plan(4, 0, 10, 5.0)


def test_python_refuses_before_anything_touches_a_device():
    import torch
    from lsm_speech_classifier_amd import frontend
    audio = torch.zeros((3, 50), dtype=torch.float32)
    ok = frontend.mix_arguments(audio, [0.0, 10.0, np.inf], rows=1, shift=[-1, 0, 1])
    assert ok[1].tolist() == [1.0, 0.1, 0.0] and ok[1].dtype == np.float64
    assert ok[2].tolist() == [1, 1, 1] and ok[2].dtype == np.int32 and ok[3] is None and ok[5] is None
    for snr in (np.nan, -np.inf, [0.0, np.nan, 1.0], [1.0, 2.0], -4000.0):
        with pytest.raises(ValueError, match="snr_db"):
            frontend.mix_arguments(audio, snr)
    with pytest.raises(ValueError, match="out must not be audio"):
        frontend.mix_arguments(audio, 10.0, out=audio)
    with pytest.raises(ValueError, match="out must not be audio"):
        frontend.mix_arguments(audio, 10.0, out=audio.view(3, 50))
    with pytest.raises(ValueError, match="out must be"):
        frontend.mix_arguments(audio, 10.0, out=torch.zeros((3, 51)))
    with pytest.raises(ValueError, match="audio must be"):
        frontend.mix_arguments(torch.zeros(50), 10.0)
    with pytest.raises(ValueError, match="audio must be"):
        frontend.mix_arguments(np.zeros((3, 50)), 10.0)                 # float64
    with pytest.raises(ValueError, match="rows"):
        frontend.mix_arguments(audio, 10.0, rows=[0, 1])
    with pytest.raises(ValueError, match="shift"):
        frontend.mix_arguments(audio, 10.0, shift=[0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="offsets"):
        frontend.mix_arguments(audio, 10.0, offsets=2 ** 31)
    for bank in (np.zeros((2, 0), dtype=np.float32), np.zeros((2, 5)), np.zeros((2, 3, 4), dtype=np.float32)):
        with pytest.raises(ValueError, match="noise bank"):
            frontend.NoiseMixer(bank)


def test_coloured_noise_is_seeded():
    from lsm_speech_classifier_amd import synth
    a, b, c = synth.coloured_noise(3, 4000, seed=1), synth.coloured_noise(3, 4000, seed=1), synth.coloured_noise(3, 4000, seed=2)
    assert a.dtype == np.float32 and a.shape == (3, 4000) and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert np.isfinite(a).all() and (a.std(axis=1) > 0).all() and np.abs(a).max() <= 1.0
    # the rows differ in colour: the share of power in the upper half of the spectrum falls from row to row
    spec = np.abs(np.fft.rfft(a.astype(np.float64), axis=1)) ** 2
    upper = spec[:, spec.shape[1] // 2:].sum(axis=1) / spec.sum(axis=1)
    assert upper[0] > upper[1] > upper[2]


def test_no_gpu_means_loud_failure_for_the_mixer():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lsm_speech_classifier_amd import _lib, frontend
    with pytest.raises(_lib.LsmHipError):
        frontend.NoiseMixer(np.zeros((2, 100), dtype=np.float32))


# ---- the scripts' flags ----------------------------------------------------------------------------------------------------
def test_main_forwards_the_corruption_flags_to_stage_1_and_nothing_without_them(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert calls[0][1:] == [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, noise_dir="synthetic", snr_db="0,20", time_shift_ms=100.0,
                          level_db="-6,0", augment_seed=7)
    assert calls[0][6:] == ["--noise-dir", "synthetic", "--snr-db", "0,20", "--level-db", "-6,0", "--time-shift-ms", "100.0",
                            "--augment-seed", "7"]
    assert calls[1][1:] == [os.path.join(ROOT, "extract_lsm_features.py"), "--feature-set", "original", "--multiplier", "0.6"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, noise_dir="synthetic", snr_db="10")
    code = calls[0][2]
    assert "'noise_dir': 'synthetic'" in code and "'snr_db': '10'" in code and "'augment_seed': 42" in code
    assert "corrupt=corrupt" in code


def test_corruption_flags_parse_into_a_plan(tmp_path):
    import argparse
    import create_dataset as cd
    from scipy.io import wavfile
    ap = argparse.ArgumentParser()
    cd.add_augment_flags(ap)
    assert cd.augment_from_args(ap.parse_args([])) is None and ap.parse_args([]).augment_seed == 42
    a = cd.augment_from_args(ap.parse_args(["--noise-dir", "synthetic", "--snr-db", "20,0", "--time-shift-ms", "100",
                                            "--level-db", "-6"]))
    assert a == dict(noise_dir="synthetic", snr_db=(0.0, 20.0), time_shift_ms=100.0, level_db=-6.0, seed=42)
    bank, plan = cd.corruption(a, 50)
    assert bank.shape == (cd.SYNTHETIC_NOISE_ROWS, cd.SYNTHETIC_NOISE_SECONDS * 16000) and bank.dtype == np.float32
    assert np.abs(plan.shift).max() <= 1600 and (plan.scale == np.float32(10 ** (-6 / 20))).all()
    assert (plan.snr_db >= 0).all() and (plan.snr_db <= 20).all()
    # a shift alone needs no noise: one silent sample, every clip clean
    bank, plan = cd.corruption(cd.augment_from_args(ap.parse_args(["--time-shift-ms", "10"])), 5)
    assert bank.shape == (1, 1) and np.isinf(plan.snr_db).all() and np.abs(plan.shift).max() <= 160
    with pytest.raises(SystemExit):
        cd.augment_from_args(ap.parse_args(["--snr-db", "10"]))         # an SNR without noise
    with pytest.raises(SystemExit):
        cd.augment_from_args(ap.parse_args(["--noise-dir", "synthetic", "--snr-db", "1,2,3"]))
    # a folder of wav files at two rates and lengths: resampled to 16 kHz, the shorter one repeated
    rng = np.random.default_rng(3)
    wavfile.write(str(tmp_path / "b_hum.wav"), 16000, (rng.standard_normal(4000) * 3000).astype(np.int16))
    wavfile.write(str(tmp_path / "a_hiss.wav"), 8000, (rng.standard_normal(3000) * 3000).astype(np.int16))
    bank = cd.load_noise_bank(str(tmp_path))
    assert bank.shape == (2, 6000) and bank.dtype == np.float32
    assert bank[1, :4000].tobytes() == cd._decode_wav(tmp_path / "b_hum.wav")[1].tobytes()
    assert bank[1, 4000:].tobytes() == bank[1, :2000].tobytes()
    with pytest.raises(ValueError, match="no readable wav"):
        cd.load_noise_bank(str(tmp_path / "nothing"))
