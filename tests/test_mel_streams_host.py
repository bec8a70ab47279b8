"""Streamed mel front end (SPEC.md 1.7): what can be checked without a GPU -- the new public header and its ctypes table,
the build identity, `frontend.mel_stream_frame_plan` against a one-by-one enumeration of complete frames, and the front-end
check `pipeline.AudioStreamBank` makes before it touches a device."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_EXPORTS = {"lsm_mel_stream_state_bytes": 3, "lsm_mel_stream_workspace": 3, "lsm_mel_stream_f32": 26}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def test_the_header_declares_exactly_the_three_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_mel_stream.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.MEL_STREAM_SYMBOLS == tuple(_lib.MEL_STREAM_SIGS) and set(_lib.MEL_STREAM_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long) %s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.MEL_STREAM_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is (_lib.c_int if result == "int" else _lib.C.c_long)
        # a pointer is a void pointer in the table, a double a double, a long a long, every other scalar an int
        for p, ctype in zip(params, args):
            want = (_lib.c_void if "*" in p else _lib.C.c_double if p.startswith("double ")
                    else _lib.C.c_long if p.startswith("long ") else _lib.c_int)
            assert ctype is want, f"{name}: {p}"
    proto = re.search(r"int lsm_mel_stream_f32\((.*?)\);", header, re.S).group(1)
    assert "const int32_t *stream_hops" in proto and "double db_lo, double db_hi" in proto
    assert "const void *state_in, void *state_out" in proto and "void *workspace, long workspace_bytes" in proto
    assert "const float *thr_on" in proto and "float *power_out, float *db_out" in proto


def test_the_other_tables_stay_as_they_are():
    from lsm_speech_classifier_amd import _lib
    assert len(_lib.EXPORTED_SYMBOLS) == 38 and len(_lib.STREAM_SIGS) == 2 and len(_lib.AUDIO_SIGS) == 2
    for table in (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS):
        assert not set(NEW_EXPORTS) & set(table)


def test_the_library_exports_the_three_symbols():
    from lsm_speech_classifier_amd import build
    path = build.lib_path()
    assert os.path.exists(path), f"{path} is not built"
    blob = open(path, "rb").read()
    for name in NEW_EXPORTS:
        assert name.encode() + b"\0" in blob, f"{name} is not in the library's symbol table"
    try:
        lib = ctypes.CDLL(path)
    except OSError:
        return                                  # no HIP runtime to resolve against here: the symbol table was read above
    for name in NEW_EXPORTS:
        assert getattr(lib, name) is not None


def test_the_build_identity_covers_the_new_header_and_sources(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_mel_stream.h" in build.PUBLIC_HEADERS and "mel_stream.hip" in build.SOURCES
    assert "mel_body.h" in build.HEADERS
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    path = inc / "lsm_hip_mel_stream.h"
    data = bytearray(path.read_bytes())
    data[len(data) // 2] ^= 1
    path.write_bytes(bytes(data))
    assert build.source_id(str(inc)) != build.source_id()


# ---- mel_stream_frame_plan against the enumeration of frames --------------------------------------------------------------
def _completed(n_hops, hop):
    """Frames t whose last sample t * hop + 1024 lies inside the first n_hops * hop samples, counted one by one."""
    t = 0
    while t * hop + 1024 <= n_hops * hop:
        t += 1
    return t


@pytest.mark.parametrize("hop", [128, 160, 256, 1024])
def test_mel_stream_frame_plan_equals_the_enumeration(hop):
    from lsm_speech_classifier_amd import frontend
    for seen in range(16):
        for new in range(16):
            want = _completed(seen + new, hop) - _completed(seen, hop)
            assert frontend.mel_stream_frame_plan(seen, new, hop) == want, (seen, new)
            assert 0 <= want <= new
    seen_a, new_a = np.meshgrid(np.arange(16), np.arange(16))
    got = frontend.mel_stream_frame_plan(seen_a, new_a, hop)
    assert got.dtype == np.int64 and got.shape == seen_a.shape
    assert got.tolist() == [[_completed(int(s) + int(n), hop) - _completed(int(s), hop) for s, n in zip(rs, rn)]
                            for rs, rn in zip(seen_a, new_a)]
    # the latency: the first frame arrives at exactly Lg = ceil(1024 / hop) hops
    lg = -(-1024 // hop)
    assert lg == {128: 8, 160: 7, 256: 4, 1024: 1}[hop]
    assert frontend.mel_stream_frame_plan(0, lg - 1, hop) == 0
    assert frontend.mel_stream_frame_plan(0, lg, hop) == 1
    assert frontend.mel_stream_frame_plan(0, lg + 5, hop, 2048) == 6


def test_mel_stream_frame_plan_refuses():
    from lsm_speech_classifier_amd import frontend
    assert frontend.mel_stream_frame_plan(0, 7) == 1                    # the defaults: hop 160, n_fft 2048
    for hop in (127, 1025):
        with pytest.raises(ValueError, match="hop"):
            frontend.mel_stream_frame_plan(0, 1, hop)
    with pytest.raises(ValueError, match="n_fft"):
        frontend.mel_stream_frame_plan(0, 1, 160, 1024)
    for seen, new in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError, match=">= 0"):
            frontend.mel_stream_frame_plan(seen, new)


# ---- AudioStreamBank's front-end check: before any device is touched -------------------------------------------------------
class _NoDevice:
    """Stands in for the reservoir: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the reservoir was touched ({name})")


class _Mel:
    filterbank = "mel"
    n_thr, n_streams, n_channels = 4, 3, 40

    def push(self, audio, hops=None):
        raise AssertionError("the front end was launched")


def test_audio_stream_bank_takes_a_streamed_mel_front_end():
    from lsm_speech_classifier_amd import frontend, pipeline

    class _Streamed(_Mel):
        streamed = True
    # past the front-end check: the next refusal is the segment length's
    with pytest.raises(ValueError, match="segment_steps"):
        pipeline.AudioStreamBank(_Streamed(), _NoDevice(), 6, 3, 1)
    with pytest.raises(ValueError, match="mel front end") as e:
        pipeline.AudioStreamBank(_Mel(), _NoDevice(), 8, 3, 1)
    assert "MelStream" in str(e.value)

    class _Truthy(_Mel):
        streamed = 1                            # `streamed is True`, not anything truthy
    with pytest.raises(ValueError, match="mel front end"):
        pipeline.AudioStreamBank(_Truthy(), _NoDevice(), 8, 3, 1)
    assert frontend.MelStream.filterbank == "mel" and frontend.MelStream.streamed is True
