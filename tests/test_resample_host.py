"""Polyphase resampler (SPEC.md 1.8): what can be checked without a GPU -- the tap table against scipy's design, the unit
arithmetic, the NumPy restatement of the arithmetic (tests/resample_restatement.py) against `scipy.signal.resample_poly`
and against itself cut into pushes, the new public header, its ctypes table and the library's exports, and the refusals the
Python layer makes before it touches a device."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_restatement as R  # noqa: E402

NEW_EXPORTS = {"lsm_resample_state_bytes": 2, "lsm_resample_f32": 12, "lsm_resample_stream_f32": 13}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("

# rate -> up, down, K, D, Hs
DESIGNS = {48000: (1, 3, 64, 11, 63), 44100: (160, 441, 9262, 11, 57), 8000: (2, 1, 42, 21, 20),
           11025: (640, 441, 13016, 15, 20), 96000: (1, 6, 127, 11, 126), 22050: (320, 441, 9262, 11, 28),
           32000: (1, 2, 43, 11, 42)}
CHECKED = (48000, 44100, 8000, 11025)


def _signal(n, seed, dtype=np.float32):
    """Seeded noise under a level ramp."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * np.linspace(0.05, 0.6, n)
    if dtype == np.int16:
        return np.clip(np.round(x * 8192), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


# ---- the design ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(DESIGNS))
def test_resample_table_is_scipys_design(rate):
    from scipy.signal import firwin
    from lsm_speech_classifier_amd import frontend
    t = frontend.resample_table(rate)
    up, down, K, D, Hs = DESIGNS[rate]
    assert (t.up, t.down, len(t.taps), t.delay, t.history) == (up, down, K, D, Hs)
    assert t.taps.dtype == np.float64 and t.pre == K - (2 * 10 * max(up, down) + 1) and not t.taps[:t.pre].any()
    assert (10 * max(up, down) + t.pre) == D * down                 # the delay is an exact integer
    ref = firwin(2 * 10 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    err = np.abs(t.taps[t.pre:] - ref).max()
    ulp = np.spacing(np.abs(ref).max())
    print(f"{rate} Hz: taps differ from firwin by {err / ulp:.3f} ulp of the largest tap")
    assert err <= 8 * ulp
    # the table laid out by phase fits a compute unit's LDS
    assert up * (-(-K // up) | 1) * 8 <= frontend.RESAMPLE_LDS_BYTES
    assert frontend.resample_table(rate, 16000).taps.tobytes() == t.taps.tobytes()


def test_unit_arithmetic():
    from lsm_speech_classifier_amd import frontend
    want = {48000: (480, 1), 44100: (441, 1), 8000: (80, 1), 11025: (441, 4)}
    for rate, (unit_in, unit_hops) in want.items():
        t = frontend.resample_table(rate)
        unit_blocks, got_in, got_hops = frontend.resample_units(t.up, t.down)
        assert (got_in, got_hops) == (unit_in, unit_hops), rate
        assert unit_blocks == 160 // np.gcd(t.up, 160) and got_in == unit_blocks * t.down
        assert unit_blocks * t.up == got_hops * 160                 # a unit is a whole number of front-end hops


# ---- the restatement of SPEC.md 1.8 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", CHECKED)
def test_restatement_against_resample_poly_and_cut_against_uncut(rate):
    from scipy.signal import resample_poly
    from lsm_speech_classifier_amd import frontend
    t = frontend.resample_table(rate)
    blocks = {48000: 500, 44100: 5, 8000: 400, 11025: 6}[rate]
    x = _signal(blocks * t.down, seed=rate)
    y = R.batch(x, t)
    ref = resample_poly(x.astype(np.float64), t.up, t.down)
    assert y.shape == ref.shape and y.dtype == np.float32
    err, bound = np.abs(y - ref).max(), 2.0 ** -23 * np.abs(ref).max()
    print(f"{rate} Hz: max |y - resample_poly| = {err:.3e} = {err / bound:.2f} of the bound {bound:.3e}")
    assert err <= bound
    # a smaller n_out is the prefix
    assert R.batch(x, t, 37).tobytes() == y[:37].tobytes()
    # z[D:] is the batch result over the same samples
    z = R.stream(x, t)
    assert len(z) == blocks * t.up
    assert z[t.delay:].tobytes() == y[:len(z) - t.delay].tobytes()
    # cut at block boundaries: a single block (shorter than the history at 48 kHz), an empty push, uneven pieces
    cuts = [1, 0, 2, blocks - 4, 1]
    zc, hist = R.stream_cut(x, t, cuts)
    assert zc.tobytes() == z.tobytes()
    assert hist.tobytes() == x[len(x) - t.history:].tobytes()
    # int16 input is the float32 input of the scaled samples
    s = _signal(blocks * t.down, seed=rate + 1, dtype=np.int16)
    assert R.batch(s, t).tobytes() == R.batch(s.astype(np.float32) / np.float32(32768.0), t).tobytes()


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_three_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_resample.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.RESAMPLE_SYMBOLS == tuple(_lib.RESAMPLE_SIGS) and set(_lib.RESAMPLE_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long) %s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.RESAMPLE_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is (_lib.c_int if result == "int" else _lib.C.c_long)
        for p, ctype in zip(params, args):                          # a pointer is a void pointer, every scalar an int
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    proto = " ".join(re.search(r"int lsm_resample_stream_f32\((.*?)\);", header, re.S).group(1).split())
    assert "const int32_t *stream_blocks" in proto and "const void *state_in, void *state_out" in proto
    for table in (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS):
        assert not set(NEW_EXPORTS) & set(table)


def test_the_library_exports_every_function_the_header_declares():
    from lsm_speech_classifier_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "lsm_hip_resample.h")).read()
    declared = set(re.findall(_DECLARED, header, re.M))
    assert declared == set(NEW_EXPORTS)
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in lsm_hip_resample.h but not exported"
    blob = open(build.lib_path(), "rb").read()
    for name in declared:
        assert name.encode() + b"\0" in blob
    assert ctypes.CDLL(build.lib_path()).lsm_resample_f32 is not None


def test_the_build_identity_covers_the_new_header_and_sources(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_resample.h" in build.PUBLIC_HEADERS and "resample.hip" in build.SOURCES
    assert "resample_body.h" in build.HEADERS
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    path = inc / "lsm_hip_resample.h"
    data = bytearray(path.read_bytes())
    data[len(data) // 2] ^= 1
    path.write_bytes(bytes(data))
    assert build.source_id(str(inc)) != build.source_id()


def test_state_bytes():
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    for rate, (up, _, K, _, Hs) in DESIGNS.items():
        n = lib.lsm_resample_state_bytes(K, up)
        assert n % 16 == 0 and Hs * 4 <= n < Hs * 4 + 16, rate
        assert frontend.resample_table(rate).history == Hs
    assert lib.lsm_resample_state_bytes(1, 1) == 16                 # no history: still a block
    for K, up in ((0, 1), (-3, 2), (64, 0), (64, -1)):
        assert lib.lsm_resample_state_bytes(K, up) == 0


# ---- refusals before a device is touched -----------------------------------------------------------------------------------
def test_bad_rates_are_refused_on_the_host(monkeypatch):
    from lsm_speech_classifier_amd import _lib, frontend

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", touched)
    monkeypatch.setattr(_lib, "load", touched)
    for rate in (0, -8000, 44100.0, "48000", None, True):
        with pytest.raises(ValueError, match="rate_in"):
            frontend.resample_table(rate)
        with pytest.raises(ValueError, match="rate_in"):
            frontend.Resampler(rate)
        with pytest.raises(ValueError, match="rate_in"):
            frontend.ResampleStream(rate, 2)
    with pytest.raises(ValueError, match="rate_out"):
        frontend.Resampler(48000, 0)
    with pytest.raises(ValueError, match="nothing to design"):
        frontend.resample_table(16000)
    # 16000 + 1 Hz: 16000 phases of 21 taps, 2.7 MB laid out by phase
    with pytest.raises(ValueError, match="LDS"):
        frontend.resample_table(16001)
    with pytest.raises(ValueError, match="LDS"):
        frontend.Resampler(16001)
    for n in (0, -1, 65536):
        with pytest.raises(ValueError, match="n_streams"):
            frontend.ResampleStream(48000, n)


def test_wrong_shapes_and_counts_are_refused_on_the_host():
    import torch
    from lsm_speech_classifier_amd import frontend
    ok = np.zeros((3, 12), dtype=np.float32)
    t, fmt = frontend.checked_pcm(ok, 3, 3)
    assert fmt == 0 and t.dtype == torch.float32 and tuple(t.shape) == (3, 12)
    t, fmt = frontend.checked_pcm(torch.zeros((2, 5), dtype=torch.int16))
    assert fmt == 1 and t.dtype == torch.int16
    for bad in (np.zeros((3, 12), dtype=np.float64), np.zeros((3, 12), dtype=np.int32), torch.zeros((3, 12), dtype=torch.float64),
                [[0.0] * 12] * 3):
        with pytest.raises(ValueError, match="float32 or int16"):
            frontend.checked_pcm(bad, 3, 3)
    for bad in (np.zeros(12, dtype=np.float32), np.zeros((2, 12), dtype=np.float32), np.zeros((3, 13), dtype=np.float32),
                np.zeros((3, 0), dtype=np.float32), np.zeros((3, 2, 6), dtype=np.float32)):
        with pytest.raises(ValueError, match=r"must be \(3, G \* 3"):
            frontend.checked_pcm(bad, 3, 3)
    with pytest.raises(ValueError, match=r"must be \(n, L >= 1\)"):
        frontend.checked_pcm(np.zeros((4, 0), dtype=np.int16))
    assert frontend.checked_counts(None, 3, 7).tolist() == [7, 7, 7]
    assert frontend.checked_counts([0, 7, 3], 3, 7).dtype == np.int64
    for bad in ([0, 8, 1], [-1, 0, 0], [1, 2], [1.0, 2.0, 3.0], 3):
        with pytest.raises(ValueError, match="blocks must be 3 integers"):
            frontend.checked_counts(bad, 3, 7)


# ---- AudioStreamBank with a resampler: the bookkeeping on CPU tensors ------------------------------------------------------
class _NoDevice:
    """Stands in for the reservoir: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the reservoir was touched ({name})")


class _FrontEnd:
    filterbank = "gammatone"
    n_thr, n_streams, n_channels, hop = 4, 2, 5, 160

    def __init__(self):
        self.calls = []

    def push(self, audio, hops=None):
        import torch
        self.calls.append((audio, np.array(hops)))
        H = audio.shape[1] // self.hop
        return torch.zeros((self.n_streams, self.n_channels, H * self.n_thr), dtype=torch.uint8), np.array(hops)

    def reset(self, slots):
        self.calls.append(("reset", list(slots)))


class _Resampler:
    """ResampleStream's surface at 11025 Hz, on the host: a unit is 441 samples in, 640 out, 4 hops."""
    n_streams, up, down, unit_blocks, unit_in, unit_hops = 2, 640, 441, 1, 441, 4

    def __init__(self):
        self.calls = []

    def push(self, audio, blocks=None):
        import torch
        self.calls.append((audio, np.array(blocks)))
        G = audio.shape[1] // self.down
        return torch.full((self.n_streams, G * self.up), 0.5), np.array(blocks) * self.up

    def reset(self, slots):
        self.calls.append(("reset", list(slots)))


class _Bank:
    def __init__(self, net, n_streams, *a):
        self.pushed, self.resets = [], []

    def push(self, rasters, segments):
        self.pushed.append((tuple(rasters.shape), np.array(segments)))
        return "rows", "counts"

    def reset(self, slots):
        self.resets.append(list(slots))


def test_audio_stream_bank_forwards_units_as_blocks_and_hops(monkeypatch):
    import torch
    from lsm_speech_classifier_amd import pipeline
    import contextlib
    monkeypatch.setattr(pipeline, "StreamBank", _Bank)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())    # the push's tensors live on the host

    class _Net:
        n_channels, device = 5, torch.device("cpu")
    fe, rs = _FrontEnd(), _Resampler()
    bank = pipeline.AudioStreamBank(fe, _Net(), 8, 3, 1, resampler=rs)
    audio = np.zeros((2, 3 * 441), dtype=np.int16)
    assert bank.push(audio, [3, 1]) == ("rows", "counts")
    (pcm, blocks), = rs.calls
    assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (2, 1323) and blocks.tolist() == [3, 1]
    (samples, hops), = fe.calls
    assert tuple(samples.shape) == (2, 3 * 640) and hops.tolist() == [12, 4]
    # 12 and 4 columns of 4 steps: 6 and 2 segments of 8 steps
    assert bank.bank.pushed[-1][1].tolist() == [6, 2] and bank.pending_steps.tolist() == [0, 0]
    bank.push(audio[:, :441], None)                                 # None: every stream delivers every unit
    assert rs.calls[-1][1].tolist() == [1, 1] and fe.calls[-1][1].tolist() == [4, 4]
    bank.reset([1])
    assert rs.calls[-1] == ("reset", [1]) and fe.calls[-1] == ("reset", [1]) and bank.bank.resets == [[1]]
    for bad_audio, bad_units, msg in ((np.zeros((2, 440), dtype=np.int16), [1, 1], "G \\* 441"),
                                      (np.zeros((3, 441), dtype=np.int16), [1, 1], "must be \\(2,"),
                                      (np.zeros((2, 441), dtype=np.float64), [1, 1], "float32 or int16"),
                                      (audio, [4, 0], "units must be 2 integers in \\[0, 3\\]"),
                                      (audio, [1], "units"), (audio, [-1, 0], "units")):
        n_rs, n_fe = len(rs.calls), len(fe.calls)
        with pytest.raises(ValueError, match=msg):
            bank.push(bad_audio, bad_units)
        assert (len(rs.calls), len(fe.calls)) == (n_rs, n_fe)           # refused before anything is pushed


def test_audio_stream_bank_refuses_a_resampler_that_does_not_fit():
    from lsm_speech_classifier_amd import pipeline

    class _Three(_Resampler):
        n_streams = 3
    with pytest.raises(ValueError, match="3 streams"):
        pipeline.AudioStreamBank(_FrontEnd(), _NoDevice(), 8, 3, 1, resampler=_Three())

    class _OtherHop(_FrontEnd):
        hop = 128
    with pytest.raises(ValueError, match="hops of the front end's 128"):
        pipeline.AudioStreamBank(_OtherHop(), _NoDevice(), 8, 3, 1, resampler=_Resampler())
