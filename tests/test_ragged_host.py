"""Ragged batches (SPEC.md 4c): what can be checked without a GPU -- `snn.ragged_chunks` against a brute-force enumeration
of every clip's steps, and the new export `lsm_reservoir_run_ragged` in the header and in the ctypes table."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [96, 0, 1, 37, 64, 95, 2, 50]


def _brute_force(lengths, chunk):
    """Launch k covers the global steps [k * chunk, (k + 1) * chunk) cut at the longest clip; clip b runs those of them
    that it has, counted one by one."""
    longest = max(lengths) if len(lengths) else 0
    launches = []
    k = 0
    while k * chunk < longest:
        first = k * chunk
        steps_here = [t for t in range(first, first + chunk) if t < longest]
        per_clip = [sum(1 for t in steps_here if t < L) for L in lengths]
        launches.append((first, len(steps_here), per_clip))
        k += 1
    return launches


@pytest.mark.parametrize("lengths,chunk", [(LENGTHS, 40), (LENGTHS, 96), (LENGTHS, 1), ([0, 0, 0], 40), ([0], 1), ([37], 40),
                                           ([37], 10), ([1], 1)])
def test_ragged_chunks_equal_the_enumeration(lengths, chunk):
    from lsm_speech_classifier_amd import snn
    got = snn.ragged_chunks(lengths, chunk)
    want = _brute_force(lengths, chunk)
    assert len(got) == len(want) == -(-max(lengths) // chunk)
    for (f, n, steps), (f_w, n_w, steps_w) in zip(got, want):
        assert (f, n) == (f_w, n_w)
        assert isinstance(steps, np.ndarray) and steps.dtype == np.int32 and steps.tolist() == steps_w
        assert 1 <= n <= chunk and steps.max() == n and steps.min() >= 0       # the longest clip fills every launch
    # every clip's steps add up to its length, and a clip that ran short of a launch gets nothing afterwards
    total = np.zeros(len(lengths), dtype=np.int64)
    ended = np.zeros(len(lengths), dtype=bool)
    for _, n, steps in got:
        assert not (steps[ended] > 0).any()
        ended |= steps < n
        total += steps
    assert total.tolist() == list(lengths)


def test_ragged_chunks_of_the_suite():
    from lsm_speech_classifier_amd import snn
    got = snn.ragged_chunks(LENGTHS, 40)
    assert [(f, n) for f, n, _ in got] == [(0, 40), (40, 40), (80, 16)]
    assert [s.tolist() for _, _, s in got] == [[40, 0, 1, 37, 40, 40, 2, 40], [40, 0, 0, 0, 24, 40, 0, 10],
                                              [16, 0, 0, 0, 0, 15, 0, 0]]
    assert snn.ragged_chunks([0, 0], 5) == [] and snn.ragged_chunks([], 5) == []
    for bad in (([3, -1], 4), ([3], 0)):
        with pytest.raises(ValueError):
            snn.ragged_chunks(*bad)


def test_the_header_declares_the_export_and_the_signature_matches():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\(", header, re.M))
    name = "lsm_reservoir_run_ragged"
    assert name in declared, f"{name} is not declared in include/lsm_hip.h"
    assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS, f"{name} has no ctypes signature"
    proto = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert len(params) == len(_lib._SIGS[name][1]) == 18
    assert _lib._SIGS[name][0] is _lib.c_int
    assert params[4] == "const int32_t *clip_steps" and params[5] == "int first_step"
    # every pointer parameter is a void pointer in the table, every scalar an int (the workspace size a long)
    for p, ctype in zip(params, _lib._SIGS[name][1]):
        want = _lib.c_void if "*" in p else (_lib.C.c_long if p.startswith("long ") else _lib.c_int)
        assert ctype is want, p
    assert len(_lib.EXPORTED_SYMBOLS) == 38
    # the launch it extends keeps its signature
    proto = re.search(r"int lsm_reservoir_run_from\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["lsm_reservoir_run_from"][1]) == 17


def test_reservoir_state_carries_ended():
    import torch
    from lsm_speech_classifier_amd import snn
    st = snn.ReservoirState(torch.zeros((3, 64), dtype=torch.uint8), 4, 2)
    assert st.ended.dtype == bool and st.ended.tolist() == [False, False, False]
    st.ended[1] = True
    st.steps_done = 7
    cl = st.clone()
    assert cl.ended.tolist() == [False, True, False] and cl.steps_done == 7
    cl.ended[0] = True
    assert st.ended.tolist() == [False, True, False]                    # a copy, not a view
