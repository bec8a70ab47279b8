"""The one-launch step with carried state and time segments (include/lsm_hip_step_state.h, SPEC.md 4f), what can be checked
without a GPU: the header declares the three names with the parameter lists the issue of this form fixed (lsm_hip_step.h's
lists with the state and segment parameters spliced in), `_lib.STEP_STATE_SIGS` binds them while `_lib.STEP_SYMBOLS` keeps its
five names, the built library exports them, the build lists the new unit, and `pipeline.step_fused_from` /
`pipeline.step_fused_segments` refuse a bad segment length and a bad state on the host, before any device work, with the
messages of `SNN.run_segments` and `SNN._check_state`."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_step_fused_state_supported", "lsm_step_fused_from_f64", "lsm_step_fused_segments_f64")
STATE = ["int first_step", "const void *state_in", "void *state_out"]
SEGMENTS = ["int segment_steps", "void *records_out", "float *segment_rows_out"]


def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_binding_and_library_carry_the_three_names():
    from lsm_speech_classifier_amd import _lib, build
    step, state = _header("lsm_hip_step.h"), _header("lsm_hip_step_state.h")
    plain, query = _params(step, "lsm_step_fused_f64"), _params(step, "lsm_step_fused_supported")
    assert _params(state, "lsm_step_fused_state_supported") == query
    at = plain.index("const int32_t *key_ids")
    run_from = plain[:at] + STATE + plain[at:]
    assert _params(state, "lsm_step_fused_from_f64") == run_from
    assert _params(state, "lsm_step_fused_segments_f64") == run_from[:-1] + SEGMENTS + run_from[-1:]
    assert run_from[-1] == "void *stream"
    for name in NEW:
        res, args = _lib.STEP_STATE_SIGS[name]
        params = _params(state, name)
        assert res is _lib.c_int and len(args) == len(params), name
        for p, ctype in zip(params, args):
            if "*" in p:
                assert ctype is _lib.c_void, f"{name}: {p}"
            elif p.startswith("long "):
                assert ctype is _lib.C.c_long, f"{name}: {p}"
            else:
                assert p.startswith("int ") and ctype is _lib.c_int, f"{name}: {p}"
    assert _lib.STEP_STATE_SYMBOLS == NEW
    assert set(_lib.STEP_SYMBOLS) == {"lsm_step_fused_supported", "lsm_step_fused_f64", "lsm_step_fused_form_supported",
                                      "lsm_step_fused_masked_f64", "lsm_step_fused_ragged_f64"}
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
        assert getattr(lib, name).argtypes == _lib.STEP_STATE_SIGS[name][1]


def test_the_build_covers_the_new_unit_and_header():
    from lsm_speech_classifier_amd import build
    assert "step_fused_state.hip" in build.SOURCES
    assert "lsm_hip_step_state.h" in build.ABI_HEADERS
    before = build.source_id()
    path = os.path.join(ROOT, "include", "lsm_hip_step_state.h")
    assert os.path.exists(path)
    # the header is hashed into the build id: the id of a tree whose include directory lacks it cannot be formed
    with pytest.raises(OSError):
        build.source_id(include_dir=os.path.join(ROOT, "lsm-speech-classifier_amd"))
    assert build.source_id() == before


class _Net:
    """What the host checks read of a reservoir: SNN's own continuation checks on a state block of 64 bytes per clip."""
    num_neurons, num_output_neurons = 8, 2

    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def state_bytes(self):
        return 64


def _shape():
    from lsm_speech_classifier_amd import snn
    _Net._continuation = snn.SNN._continuation
    _Net._check_state = snn.SNN._check_state
    return types.SimpleNamespace(n_filters=128, time_bins=15, n_samples=2400, n_steps=60), _Net()


def test_step_fused_segments_refuses_a_segment_length_that_does_not_divide_the_steps():
    from lsm_speech_classifier_amd import _lib, pipeline
    fe, net = _shape()
    audio = np.zeros((3, 2400), dtype=np.float32)
    for bad in (0, -4, 7, 61, 120):
        with pytest.raises(_lib.LsmHipError, match=rf"segment_steps = {bad} must be >= 1 and divide the clip's 60 steps"):
            pipeline.step_fused_segments(fe, net, audio, bad)


def test_the_state_is_checked_before_any_device_work():
    import torch
    from lsm_speech_classifier_amd import _lib, pipeline, snn
    fe, net = _shape()
    audio = np.zeros((3, 2400), dtype=np.float32)
    good = snn.ReservoirState(torch.zeros((3, 64), dtype=torch.uint8), 8, 2)
    for call in (lambda **kw: pipeline.step_fused_from(fe, net, audio, **kw),
                 lambda **kw: pipeline.step_fused_segments(fe, net, audio, 20, **kw)):
        with pytest.raises(_lib.LsmHipError, match="state must be a ReservoirState .SNN.new_state., got Tensor"):
            call(state=good.data)
        with pytest.raises(_lib.LsmHipError, match=r"state must hold a contiguous uint8 \(3, 64\) tensor on cpu, got "
                                                   r"torch.uint8 \(2, 64\)"):
            call(state=snn.ReservoirState(torch.zeros((2, 64), dtype=torch.uint8), 8, 2))
        with pytest.raises(_lib.LsmHipError, match=r"state must hold a contiguous uint8 \(3, 64\).*got torch.int8"):
            call(state=snn.ReservoirState(torch.zeros((3, 64), dtype=torch.int8), 8, 2))
        with pytest.raises(_lib.LsmHipError, match=r"state must hold a contiguous uint8 \(3, 64\).*\(3, 48\)"):
            call(state=good, state_out=snn.ReservoirState(torch.zeros((3, 48), dtype=torch.uint8), 8, 2))
        with pytest.raises(ValueError, match="state_out needs state"):
            call(state_out=good)
    assert good.steps_done == 0


def test_the_hot_path_and_long_audio_routes_are_opt_in():
    import inspect
    from lsm_speech_classifier_amd import pipeline
    assert inspect.signature(pipeline.features_from_long_audio).parameters["fused"].default is False
    assert inspect.signature(pipeline.sliding_features_from_long_audio).parameters["fused"].default is False
    assert inspect.signature(pipeline.HotPath.__init__).parameters["fused_forms"].default is False
    assert pipeline.STEP_FORMS == {"plain": 0, "masked": 1, "ragged": 2}
