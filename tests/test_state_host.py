"""Host side of the continued reservoir runs: how a long run is cut into launches (`snn.split_steps`) and the three
exports behind it (include/lsm_hip.h against `_lib._SIGS`).  No GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("lsm_reservoir_state_bytes", "lsm_reservoir_run_from", "lsm_reservoir_max_steps")


def _covers(chunks, n_steps, max_steps):
    """Consecutive, non-empty, none longer than max_steps, all of [0, n_steps)."""
    at = 0
    for t0, n in chunks:
        assert t0 == at and 1 <= n <= max_steps, (chunks, n_steps, max_steps)
        at += n
    assert at == n_steps
    return True


def test_split_steps_edge_cases():
    from lsm_speech_classifier_amd.snn import MAX_STEPS, split_steps
    assert split_steps(96, 400) == [(0, 96)]                              # shorter than a launch: one launch
    assert split_steps(400, 400) == [(0, 400)]
    assert split_steps(1200, 400) == [(0, 400), (400, 400), (800, 400)]   # exact multiple: no empty tail
    assert split_steps(401, 400) == [(0, 400), (400, 1)]
    assert split_steps(5, 1) == [(t, 1) for t in range(5)]
    assert split_steps(0, 7) == []
    assert MAX_STEPS == 65535
    for max_steps in (1, 2, 999, 32767, 32768, 65534, 65535, 70000):
        chunks = split_steps(MAX_STEPS, max_steps)
        assert _covers(chunks, MAX_STEPS, max_steps)
        assert len(chunks) == -(-MAX_STEPS // max_steps)
        assert all(n == max_steps for _, n in chunks[:-1])                # every launch but the last is full
    for bad in ((5, 0), (5, -1), (-1, 4)):
        with pytest.raises(ValueError):
            split_steps(*bad)


def test_header_and_binding_carry_the_new_exports():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    declared = dict((name, ret) for ret, name in
                    re.findall(r"^\s*(int|long)\s+(lsm_[a-z0-9_]+)\s*\(", header, re.M))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/lsm_hip.h"
        assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS, f"{name} has no ctypes signature"
    assert declared["lsm_reservoir_state_bytes"] == "long" and _lib._SIGS["lsm_reservoir_state_bytes"][0] is _lib.C.c_long
    # the launch: as many ctypes arguments as the prototype has parameters
    proto = re.search(r"int lsm_reservoir_run_from\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["lsm_reservoir_run_from"][1]) == 17
    proto = re.search(r"int lsm_reservoir_max_steps\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["lsm_reservoir_max_steps"][1]) == 3
