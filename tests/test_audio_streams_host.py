"""Streamed gammatone front end (SPEC.md 1.6): what can be checked without a GPU -- the new public header and its ctypes
table, the build identity, `frontend.stream_column_plan` against a brute-force enumeration of completed windows, and the
refusals `pipeline.AudioStreamBank` makes before it touches a device."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_EXPORTS = {"lsm_gammatone_stream_state_bytes": 3, "lsm_gammatone_stream_f64": 21}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def test_the_header_declares_exactly_the_two_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_audio.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NEW_EXPORTS)
    assert _lib.AUDIO_SYMBOLS == tuple(_lib.AUDIO_SIGS) and set(_lib.AUDIO_SYMBOLS) == set(NEW_EXPORTS)
    for name, n_params in NEW_EXPORTS.items():
        result, proto = re.search(r"^(int|long) %s\((.*?)\);" % name, header, re.S | re.M).groups()
        params = [p.strip() for p in proto.split(",")]
        res, args = _lib.AUDIO_SIGS[name]
        assert len(params) == len(args) == n_params, name
        assert res is (_lib.c_int if result == "int" else _lib.C.c_long)
        # a pointer is a void pointer in the table, a double a double, every other scalar an int
        for p, ctype in zip(params, args):
            want = _lib.c_void if "*" in p else (_lib.C.c_double if p.startswith("double ") else _lib.c_int)
            assert ctype is want, f"{name}: {p}"
    proto = re.search(r"int lsm_gammatone_stream_f64\((.*?)\);", header, re.S).group(1)
    assert "const int32_t *stream_hops" in proto and "double db_lo, double db_hi" in proto
    assert "const void *state_in, void *state_out" in proto and "workspace" not in proto


def test_the_other_tables_stay_as_they_are():
    from lsm_speech_classifier_amd import _lib
    assert len(_lib.EXPORTED_SYMBOLS) == 38 and len(_lib.STREAM_SIGS) == 2
    for table in (_lib._SIGS, _lib.STREAM_SIGS):
        assert not set(NEW_EXPORTS) & set(table)


def test_the_library_exports_both_symbols():
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


def test_the_build_identity_covers_the_new_header_and_source(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_audio.h" in build.PUBLIC_HEADERS and "frontend_stream.hip" in build.SOURCES
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    path = inc / "lsm_hip_audio.h"
    data = bytearray(path.read_bytes())
    data[len(data) // 2] ^= 1
    path.write_bytes(bytes(data))
    assert build.source_id(str(inc)) != build.source_id()


# ---- stream_column_plan against the enumeration of windows ---------------------------------------------------------------
def _completed(n_hops, nwin, hop):
    """Windows [c * hop, c * hop + nwin) that lie inside the first n_hops * hop samples, counted one by one."""
    c = 0
    while c * hop + nwin <= n_hops * hop:
        c += 1
    return c


@pytest.mark.parametrize("nwin,hop", [(400, 160), (320, 160), (160, 160), (640, 160)])
def test_stream_column_plan_equals_the_enumeration(nwin, hop):
    from lsm_speech_classifier_amd import frontend
    for seen in range(13):
        for new in range(13):
            want = _completed(seen + new, nwin, hop) - _completed(seen, nwin, hop)
            assert frontend.stream_column_plan(seen, new, nwin, hop) == want, (seen, new)
            assert 0 <= want <= new
    seen_a, new_a = np.meshgrid(np.arange(13), np.arange(13))
    got = frontend.stream_column_plan(seen_a, new_a, nwin, hop)
    assert got.dtype == np.int64 and got.shape == seen_a.shape
    assert got.tolist() == [[_completed(int(s) + int(n), nwin, hop) - _completed(int(s), nwin, hop) for s, n in zip(rs, rn)]
                            for rs, rn in zip(seen_a, new_a)]
    # the latency: a column needs ceil(nwin / hop) hops
    assert frontend.stream_column_plan(0, -(-nwin // hop) - 1, nwin, hop) == 0
    assert frontend.stream_column_plan(0, -(-nwin // hop), nwin, hop) == 1


def test_stream_column_plan_refuses():
    from lsm_speech_classifier_amd import frontend
    assert frontend.stream_column_plan(0, 3) == 1                       # the defaults: nwin 400, hop 160
    for nwin, hop in ((641, 160), (159, 160), (400, 0)):
        with pytest.raises(ValueError, match="nwin"):
            frontend.stream_column_plan(0, 1, nwin, hop)
    for seen, new in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError, match=">= 0"):
            frontend.stream_column_plan(seen, new)


# ---- AudioStreamBank's refusals: before any device is touched --------------------------------------------------------------
class _NoDevice:
    """Stands in for the reservoir: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the reservoir was touched ({name})")


class _FrontEnd:
    filterbank = "gammatone"
    n_thr, n_streams, n_channels = 4, 3, 64

    def push(self, audio, hops=None):
        raise AssertionError("the front end was launched")


def test_audio_stream_bank_refuses_on_the_host():
    from lsm_speech_classifier_amd import pipeline
    for S in (6, 0, -4, 10):
        with pytest.raises(ValueError, match="segment_steps"):
            pipeline.AudioStreamBank(_FrontEnd(), _NoDevice(), S, 3, 1)
    with pytest.raises(ValueError, match="hop_segments"):
        pipeline.AudioStreamBank(_FrontEnd(), _NoDevice(), 8, 3, 4)
    with pytest.raises(ValueError, match="window_segments"):
        pipeline.AudioStreamBank(_FrontEnd(), _NoDevice(), 8, 0, 1)

    class _Mel(_FrontEnd):
        filterbank = "mel"
    with pytest.raises(ValueError, match="mel front end"):
        pipeline.AudioStreamBank(_Mel(), _NoDevice(), 8, 3, 1)
