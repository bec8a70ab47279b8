"""The masked and the ragged one-launch step (include/lsm_hip_step.h), what can be checked without a GPU: the header declares
the three new names, `_lib.STEP_SIGS` binds them with the header's parameter lists, the built library exports them, the build
id covers the new translation units, and `pipeline.step_fused(mask=...)` / `pipeline.step_fused_ragged` refuse a bad mask and
bad bins on the host, before any device work, with the messages of `checked_mask` and of `encode_ragged`."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_step_fused_form_supported", "lsm_step_fused_masked_f64", "lsm_step_fused_ragged_f64")


def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _header():
    return open(os.path.join(ROOT, "include", "lsm_hip_step.h")).read()


def test_header_binding_and_library_carry_the_three_names():
    from lsm_speech_classifier_amd import _lib, build
    header = _header()
    plain, query = _params(header, "lsm_step_fused_f64"), _params(header, "lsm_step_fused_supported")
    assert _params(header, "lsm_step_fused_form_supported") == query + ["int form"]
    assert _params(header, "lsm_step_fused_masked_f64") == \
        plain[:-1] + ["const uint32_t *freq_mask", "const uint32_t *time_mask"] + plain[-1:]
    at = plain.index("int time_bins") + 1
    assert _params(header, "lsm_step_fused_ragged_f64") == plain[:at] + ["const int32_t *clip_bins"] + plain[at:]
    for name in NEW + ("lsm_step_fused_supported", "lsm_step_fused_f64"):
        res, args = _lib.STEP_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params), name
        for p, ctype in zip(params, args):
            if "*" in p:
                assert ctype is _lib.c_void, f"{name}: {p}"
            elif p.startswith("long "):
                assert ctype is _lib.C.c_long, f"{name}: {p}"
            else:
                assert p.startswith("int ") and ctype is _lib.c_int, f"{name}: {p}"
    assert set(_lib.STEP_SYMBOLS) == set(NEW) | {"lsm_step_fused_supported", "lsm_step_fused_f64"}
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name


def test_the_build_covers_the_new_units():
    from lsm_speech_classifier_amd import build
    for src in ("step_fused.hip", "step_fused_masked.hip", "step_fused_ragged.hip"):
        assert src in build.SOURCES
    for inc in ("step_fused_family.inc", "step_fused_forms.h", "step_fused_tail.inc", "step_fused_bits.inc"):
        assert inc in build.HEADERS
    listed = set(build.SOURCES + build.HEADERS)
    for name in os.listdir(os.path.join(ROOT, "lsm-speech-classifier_amd", "csrc")):
        if name.startswith("step_fused"):
            assert name in listed, f"{name} is not hashed into the build id"


def _shape():
    """What the host checks read of a front end: 128 filters, 16 bins of 160 samples."""
    return types.SimpleNamespace(n_filters=128, time_bins=16, n_samples=2560), object()


def test_step_fused_refuses_a_bad_mask_before_any_device_work():
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net = _shape()
    audio = np.zeros((3, 2560), dtype=np.float32)
    with pytest.raises(ValueError, match="mask must be a frontend.MaskPlan, got tuple"):
        pipeline.step_fused(fe, net, audio, mask=(None, None))
    good = frontend.mask_plan(3, 128, 16, freq_masks=1, freq_width=8, time_masks=1, time_width=4)
    assert frontend.checked_mask(good, 3, 128, 16)
    with pytest.raises(ValueError, match=r"mask.freq must be uint32 \(3, 4\) \(one row of words per clip\), got uint32 \(2, 4\)"):
        pipeline.step_fused(fe, net, audio, mask=good.part(0, 2))
    with pytest.raises(ValueError, match=r"mask.time must be uint32 \(3, 1\)"):
        pipeline.step_fused(fe, net, audio, mask=frontend.MaskPlan(good.freq, np.zeros((3, 2), dtype=np.uint32)))
    with pytest.raises(ValueError, match=r"mask.freq must be uint32 \(3, 4\).*got int32"):
        pipeline.step_fused(fe, net, audio, mask=frontend.MaskPlan(good.freq.view(np.int32), good.time))


def test_step_fused_ragged_refuses_bad_bins_and_a_front_end_that_is_not_ragged():
    import torch
    from lsm_speech_classifier_amd import pipeline
    fe, net = _shape()
    audio = np.zeros((3, 2560), dtype=np.float32)
    with pytest.raises(ValueError, match=r"bins \[2, 17\] of clips \[0, 2\]: a clip has 0 or 3 \.\. 16 time bins"):
        pipeline.step_fused_ragged(fe, net, audio, [2, 16, 17])
    with pytest.raises(ValueError, match=r"bins \[-1\] of clips \[1\]"):
        pipeline.step_fused_ragged(fe, net, audio, [0, -1, 3])
    with pytest.raises(ValueError, match=r"bins must be 3 integers, got int64 \(2,\)"):
        pipeline.step_fused_ragged(fe, net, audio, [3, 4])
    with pytest.raises(ValueError, match=r"bins must be 3 integers, got float64"):
        pipeline.step_fused_ragged(fe, net, audio, [3.0, 4.0, 5.0])
    with pytest.raises(ValueError, match=r"bins must hold 3 int32 values, got torch.int64"):
        pipeline.step_fused_ragged(fe, net, audio, torch.tensor([3, 4, 5]))
    short = types.SimpleNamespace(n_filters=128, time_bins=16, n_samples=2500)
    with pytest.raises(ValueError, match="ragged batches take 160 samples per time bin"):
        pipeline.step_fused_ragged(short, net, audio[:, :2500], [3, 4, 5])
    two = types.SimpleNamespace(n_filters=128, time_bins=2, n_samples=320)
    with pytest.raises(ValueError, match="ragged batches need time_bins >= 3"):
        pipeline.step_fused_ragged(two, net, audio[:, :320], [0, 0, 0])


def test_the_form_names():
    from lsm_speech_classifier_amd import pipeline
    assert pipeline.STEP_FORMS == {"plain": 0, "masked": 1, "ragged": 2}
    with pytest.raises(ValueError, match="form must be one of"):
        pipeline.step_fused_supported(None, None, 1, form="both")
