"""Silence trimming (SPEC.md 1.15, include/lsm_hip_trim.h), what can be checked without a GPU: the NumPy restatement
(tests/trim_restatement.py) against a plain Python loop, its padding invariance, the header, binding and build lists, the
launch function's refusals (made before any device work, so they run here), the shared clamp and endpoint arithmetic under
AddressSanitizer as a host program, the flags of create_dataset.py and main.py, and the synthetic corpus' noise keyword."""
import argparse
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_restatement as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_trim_lds_bytes", "lsm_trim_silence_f32")
HOP = 160


# ---- the restatement against the definition written as loops ---------------------------------------------------------------
def _loop_trim(x, count, time_bins, ratio, pad_bins, min_bins, n_out):
    """SPEC.md 1.15 for one clip, one Python statement per sentence of the text."""
    n_samples = len(x)
    length = n_samples if count is None else min(max(int(count), 0), n_samples)
    nb = min((length + HOP - 1) // HOP, time_bins)
    e = []
    for j in range(nb):
        acc = np.float64(0.0)
        for i in range(HOP):
            at = HOP * j + i
            v = np.float64(x[at]) if at < length else np.float64(0.0)
            acc = acc + v * v
        e.append(acc)
    whole = nb < 3 or not all(np.isfinite(v) for v in e)
    active = []
    if not whole:
        level = max(e) * np.float64(ratio)
        active = [j for j in range(nb) if e[j] > level]
        whole = not active
    if whole:
        first, bins = 0, nb
    else:
        lo, hi = max(active[0] - pad_bins, 0), min(active[-1] + pad_bins, nb - 1)
        m = min(min_bins, nb)
        if hi - lo + 1 < m:
            need = m - (hi - lo + 1)
            g = min(need, nb - 1 - hi)
            hi, lo = hi + g, lo - (need - g)
        first, bins = lo, hi - lo + 1
    out = np.zeros(n_out, dtype=np.float32)
    for m_ in range(HOP * bins):
        at = HOP * first + m_
        if at < length:
            out[m_] = x[at]
    energy = np.zeros(time_bins, dtype=np.float64)
    energy[:nb] = e
    return out, first, bins, energy


def _speech(n_bins, spans, seed, level=0.3, floor=0.0):
    """A clip of n_bins bins: noise of ``level`` in the [lo, hi) bin spans, noise of ``floor`` elsewhere."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n_bins * HOP) * floor).astype(np.float32)
    for lo, hi in spans:
        x[HOP * lo:HOP * hi] = (rng.standard_normal(HOP * (hi - lo)) * level).astype(np.float32)
    return x


def test_the_restatement_equals_the_loops_on_small_cases():
    with np.errstate(all="ignore"):
        cases = []
        x = _speech(7, [(2, 4)], 1, floor=0.001)
        cases += [(x, None, 7, 1e-3, 1, 3), (x, 700, 7, 1e-3, 0, 3), (x, 481, 7, 0.0, 0, 3), (x, -5, 7, 0.5, 0, 3),
                  (x, 10 ** 9, 7, 0.5, 9, 3), (x, 321, 7, 1e-3, 0, 7), (x, 320, 7, 1e-3, 0, 3), (x, None, 5, 1e-3, 0, 4)]
        y = x.copy()
        y[HOP * 6 + 3] = np.nan
        cases += [(y, None, 7, 1e-3, 0, 3), (y, HOP * 6, 7, 1e-3, 0, 3)]
        cases += [(np.zeros(5 * HOP, dtype=np.float32), None, 5, 1e-3, 0, 3), (_speech(6, [(5, 6)], 2), None, 6, 0.0, 0, 3),
                  (_speech(6, [(0, 1)], 3), None, 6, 0.0, 0, 4), (_speech(6, [(0, 1)], 3)[:-3], None, 6, 0.0, 1, 3)]
        for x, count, tb, ratio, pad, minb in cases:
            n_out = HOP * tb + 3
            got = TR.trim(x[None, :], None if count is None else [count], tb, ratio, pad, minb, n_out)
            want = _loop_trim(x, count, tb, ratio, pad, minb, n_out)
            assert got[0][0].tobytes() == want[0].tobytes()
            assert (int(got[1][0]), int(got[2][0])) == (want[1], want[2])
            assert got[3][0].tobytes() == want[3].tobytes()
    # the cases are not all "kept whole"
    out, first, bins, _ = TR.trim(_speech(7, [(2, 4)], 1, floor=0.001)[None, :], None, 7, 1e-3, 1, 3)
    assert (int(first[0]), int(bins[0])) == (1, 4)


def test_the_pinned_order_is_not_numpys_pairwise_sum():
    x = _speech(50, [(0, 50)], 5)
    e = TR.energies(x, len(x), 50)
    pairwise = (x.astype(np.float64).reshape(50, HOP) ** 2).sum(axis=1)
    assert np.allclose(e, pairwise, rtol=1e-12) and (e != pairwise).any()


def test_exact_zero_padding_moves_first_and_nothing_else():
    """pad_bins = 0: whole bins of exact zeros in front of or behind a clip leave the trimmed samples and `bins` as they are,
    and `first` moves by the bins added in front."""
    core = _speech(9, [(1, 3), (5, 8)], 7, floor=0.0005)
    base = TR.trim(core[None, :], None, 9, 1e-3, 0, 3, HOP * 20)
    assert 3 <= int(base[2][0]) < 9
    for front, back in ((0, 4), (3, 0), (5, 6)):
        padded = np.concatenate([np.zeros(HOP * front, np.float32), core, np.zeros(HOP * back, np.float32)])
        out, first, bins, _ = TR.trim(padded[None, :], None, 20, 1e-3, 0, 3, HOP * 20)
        assert out.tobytes() == base[0].tobytes() and int(bins[0]) == int(base[2][0])
        assert int(first[0]) == int(base[1][0]) + front
    cut, firsts, counts = TR.slices([core, np.concatenate([np.zeros(HOP * 2, np.float32), core])], 30.0, 0, 3)
    assert cut[0].tobytes() == cut[1].tobytes() and firsts[1] == firsts[0] + 2 and counts[0] == counts[1]


# ---- header, binding, build ---------------------------------------------------------------------------------------------
def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_binding_and_library_carry_the_two_names():
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_trim.h")).read()
    assert _params(header, "lsm_trim_lds_bytes") == ["int time_bins"]
    assert _params(header, "lsm_trim_silence_f32") == [
        "const float *audio", "int n_clips", "int n_samples", "int time_bins", "const int32_t *clip_samples", "double ratio",
        "int pad_bins", "int min_bins", "float *audio_out", "int n_samples_out", "int32_t *clip_first_out",
        "int32_t *clip_bins_out", "double *energy_out", "void *stream"]
    assert _lib.TRIM_SYMBOLS == tuple(_lib.TRIM_SIGS) == NEW
    for name in NEW:
        res, args = _lib.TRIM_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params)
        for p, ctype in zip(params, args):
            want = _lib.c_void if "*" in p else _lib.c_double if p.startswith("double ") else _lib.c_int
            assert ctype is want, f"{name}: {p}"
    assert len(_lib.EXPORTED_SYMBOLS) == 38 and not set(NEW) & set(_lib._SIGS)
    tables = [_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
              _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS, _lib.RAGGED_SIGS, _lib.STEP_SIGS,
              _lib.STEP_STATE_SIGS, _lib.TRIM_SIGS]
    assert sum(len(t) for t in tables) == 77 and len(set().union(*tables)) == 77        # 77 exports over fourteen headers
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert "trim.hip" in build.SOURCES and "trim_body.h" in build.HEADERS and "lsm_hip_trim.h" in build.ABI_HEADERS
    assert len(build.PUBLIC_HEADERS) == 9
    with pytest.raises(OSError):                                    # the header is hashed into the build id
        build.source_id(include_dir=os.path.join(ROOT, "lsm-speech-classifier_amd"))


def test_lds_bytes_and_the_refusals_in_their_order():
    """Every refusal is made on the host before anything is launched, so fake (aligned, distinct) addresses serve."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    assert lib.lsm_trim_lds_bytes(2) < 0 and lib.lsm_trim_lds_bytes(4097) < 0
    assert lib.lsm_trim_lds_bytes(3) == 8 * 3 + 4 * 64 * 161 and lib.lsm_trim_lds_bytes(4096) == 8 * 4096 + 4 * 64 * 161
    assert lib.lsm_trim_lds_bytes(4096) <= 160 * 1024
    A, O, L, F, B, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    good = dict(audio=A, n_clips=2, n_samples=500, time_bins=4, clip_samples=L, ratio=1e-3, pad_bins=1, min_bins=3,
                audio_out=O, n_samples_out=640, first=F, bins=B, energy=E)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_trim_silence_f32(a["audio"] or None, a["n_clips"], a["n_samples"], a["time_bins"], a["clip_samples"] or None,
                                      C.c_double(a["ratio"]), a["pad_bins"], a["min_bins"], a["audio_out"] or None,
                                      a["n_samples_out"], a["first"] or None, a["bins"] or None, a["energy"] or None, None)
        return rc, lib.lsm_last_error().decode()

    # each row breaks its own rule AND every later one: the message names the earliest
    later = [dict(n_clips=-1), dict(time_bins=2), dict(ratio=float("nan")), dict(pad_bins=-1), dict(min_bins=2),
             dict(audio=0), dict(audio_out=A), dict(n_samples_out=639), dict(energy=E + 4)]
    texts = ["n_clips=-1", "time_bins=2 must be", "ratio=", "pad_bins=-1", "min_bins=2 outside", "are required", "must not be audio",
             "n_samples_out=639", "8-byte aligned"]
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)
    for kw, text, code in ((dict(n_samples=0), "n_samples=0", -1), (dict(time_bins=4097, min_bins=3), "4096", -4),
                           (dict(ratio=1.0), "ratio=1", -1), (dict(ratio=-0.5), "ratio=-0.5", -1),
                           (dict(ratio=float("inf")), "ratio=inf", -1), (dict(min_bins=5), "min_bins=5 outside", -1),
                           (dict(audio_out=0), "are required", -1), (dict(audio=A + 2), "4-byte aligned", -1),
                           (dict(audio_out=O + 1), "4-byte aligned", -1), (dict(clip_samples=L + 2), "4-byte aligned", -1),
                           (dict(first=F + 1), "4-byte aligned", -1), (dict(bins=B + 3), "4-byte aligned", -1)):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert call(n_clips=0)[0] == 0                                   # nothing to do, nothing launched


def test_the_clamp_and_endpoint_arithmetic_under_address_sanitizer(tmp_path):
    """csrc/trim_body.h -- the code the kernel forms every address with -- as a host program over the count corners, built
    with -fsanitize=address,undefined (tests/trim_body_check.cc)."""
    src = os.path.join(ROOT, "tests", "trim_body_check.cc")
    exe = str(tmp_path / "trim_body_check")
    built = False
    # the runtimes are linked statically: the program then needs nothing of the environment it is started from
    for cxx, static in ((shutil.which("g++"), ["-static-libasan", "-static-libubsan"]), (shutil.which("clang++"), [])):
        if not cxx:
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
                           + ["-I", os.path.join(ROOT, "lsm-speech-classifier_amd", "csrc"), src, "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            built = True
            break
    if not built:
        pytest.skip("no host compiler with the sanitizer runtimes")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "trim_body ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the Python layer's host checks ---------------------------------------------------------------------------------------
def test_trim_ratio():
    from lsm_speech_classifier_amd import frontend
    assert frontend.trim_ratio(None) == 0.0 and frontend.trim_ratio(30.0) == 10.0 ** -3.0 == TR.ratio_of(30.0)
    assert frontend.trim_ratio(10) == TR.ratio_of(10) and 0.0 < frontend.trim_ratio(200.0) < 1.0
    for bad in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="top_db"):
            frontend.trim_ratio(bad)


# ---- the scripts' flags ---------------------------------------------------------------------------------------------------
def _parser(cd):
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--resample", default="host")
    for add in (cd.add_augment_flags, cd.add_reverb_flags, cd.add_speed_flags, cd.add_mask_flags, cd.add_variable_length_flags):
        add(ap)
    return ap


def test_trim_flags_parse_refuse_and_forward(monkeypatch):
    import create_dataset as cd
    import main as pipeline
    ap = _parser(cd)
    none = ap.parse_args([])
    assert none.trim_silence is None and none.trim_pad_ms == 30.0 and none.trim_min_ms == 30.0
    assert cd.trim_from_args(none) is None and cd.trim_from_args(ap.parse_args(["--variable-length"])) is None
    a = ap.parse_args(["--variable-length", "--trim-silence", "30"])
    cd.check_variable_length_args(a)
    assert cd.trim_from_args(a) == dict(top_db=30.0, pad_bins=3, min_bins=3)
    a = ap.parse_args(["--variable-length", "--trim-silence", "25.5", "--trim-pad-ms", "47", "--trim-min-ms", "200"])
    assert cd.trim_from_args(a) == dict(top_db=25.5, pad_bins=5, min_bins=20)
    with pytest.raises(SystemExit, match="--trim-silence needs --variable-length"):
        cd.trim_from_args(ap.parse_args(["--trim-silence", "30"]))
    for bad, text in ((["--trim-silence", "0"], "--trim-silence must be"), (["--trim-silence", "-3"], "--trim-silence must be"),
                      (["--trim-silence", "30", "--trim-pad-ms", "-1"], "--trim-pad-ms"),
                      (["--trim-silence", "30", "--trim-min-ms", "10"], "--trim-min-ms"),
                      (["--trim-silence", "30", "--trim-min-ms", "600", "--max-seconds", "0.5"], "--trim-min-ms")):
        with pytest.raises(SystemExit, match=text):
            cd.trim_from_args(ap.parse_args(["--variable-length"] + bad))
    # the script itself refuses the flag without its route, before any device work
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--trim-silence", "30", "--synthetic-per-class", "1"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "--trim-silence needs --variable-length" in r.stderr
    # main.py forwards the three flags with --variable-length and nothing without --trim-silence
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, *k, **kw: calls.append(cmd) or 0)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, max_seconds=0.5)
    assert calls[0][6:] == ["--variable-length", "--max-seconds", "0.5"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, trim_silence=30.0, trim_pad_ms=20.0)
    assert calls[0][6:] == ["--variable-length", "--max-seconds", "1.0", "--trim-silence", "30.0", "--trim-pad-ms", "20.0",
                            "--trim-min-ms", "30.0"]
    with pytest.raises(SystemExit, match="--trim-silence needs --variable-length"):
        pipeline.run_pipeline(128, "gammatone", "original", 0.6, trim_silence=30.0)


# ---- the synthetic corpus ---------------------------------------------------------------------------------------------------
def test_class_chirps_noise_keyword_defaults_to_todays_bytes_and_quiet_clips_trim():
    import inspect
    from lsm_speech_classifier_amd import synth
    assert inspect.signature(synth.class_chirps).parameters["noise"].default == 0.04
    labels = [0, 5, 11]
    today = synth.class_chirps(labels, seed=1234)
    assert synth.class_chirps(labels, seed=1234, noise=0.04).tobytes() == today.tobytes()
    quiet = synth.class_chirps(labels, seed=1234, noise=0.001)
    # the same draws at another level: the difference of the two is the noise, scaled
    noise = today.astype(np.float64) - quiet.astype(np.float64)
    assert abs(noise.std() - 0.039) < 2e-3
    _, _, bins = TR.slices(list(quiet), 30.0, 3, 3)
    assert (bins >= 40).all() and (bins <= 70).all()                # every clip trims; none is kept whole
    _, _, loud = TR.slices(list(today), 30.0, 3, 3)
    assert (loud == 100).all()                                      # at 0.04 the background lies 10 dB under the peak bin
