"""Ragged audio (SPEC.md 1.14): what can be checked without a GPU -- `frontend.pack_utterances`, the host checks of
`SpikeFrontEnd.encode_ragged`'s ``bins`` and of the front end's shape, the new public header against its ctypes table and the
library's exports, and the build id's cover of the header."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("lsm_spec_to_spikes_ragged_f64", "lsm_spec_to_spikes_ragged_f32", "lsm_power_to_db_ragged_f32",
         "lsm_gammatone_spikes_ragged_f64")
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def _params(header: str, name: str):
    proto = re.search(r"^int\s+%s\((.*?)\);" % name, header, re.S | re.M).group(1)
    return [" ".join(p.split()) for p in proto.split(",")]


# ---- pack_utterances -------------------------------------------------------------------------------------------------------
def test_pack_utterances_pads_to_whole_bins_and_keeps_the_order():
    from lsm_speech_classifier_amd import frontend
    rng = np.random.default_rng(3)
    lens = [480, 1920, 481, 959, 960, 961, 321]
    utts = [rng.standard_normal(n).astype(np.float64 if i % 2 else np.float32) for i, n in enumerate(lens)]
    audio, bins = frontend.pack_utterances(utts, 12)
    assert audio.dtype == np.float32 and audio.shape == (7, 1920) and audio.flags.c_contiguous
    assert bins.dtype == np.int32 and bins.tolist() == [3, 12, 4, 6, 6, 7, 3]         # ceil(len / 160)
    for r, u in enumerate(utts):
        assert np.array_equal(audio[r, :len(u)], u.astype(np.float32))
        assert not audio[r, len(u):].any()
    assert frontend.RAGGED_HOP == frontend.STREAM_HOP == 160
    # a list, a tuple and int16 samples are arrays too; no utterance: an empty batch
    a2, b2 = frontend.pack_utterances([list(range(400)), np.arange(500, dtype=np.int16)], 5)
    assert a2.shape == (2, 800) and b2.tolist() == [3, 4] and a2[0, 399] == 399.0 and a2[1, 499] == 499.0
    a0, b0 = frontend.pack_utterances([], 7)
    assert a0.shape == (0, 1120) and b0.shape == (0,)


def test_pack_utterances_refuses_with_the_index_of_the_offender():
    from lsm_speech_classifier_amd import frontend
    ok = np.zeros(500, np.float32)
    with pytest.raises(ValueError, match="utterance 1 .*320 samples = 2 time bins"):
        frontend.pack_utterances([ok, np.zeros(320, np.float32)], 10)                # shorter than 3 bins
    with pytest.raises(ValueError, match="utterance 2 .*1601 samples = 11 time bins"):
        frontend.pack_utterances([ok, ok, np.zeros(1601, np.float32)], 10)           # longer than max_bins
    with pytest.raises(ValueError, match="utterance 0 must be a 1-D array"):
        frontend.pack_utterances([np.zeros((2, 500), np.float32)], 10)
    with pytest.raises(ValueError, match="utterance 1 .*0 samples"):
        frontend.pack_utterances([ok, np.zeros(0, np.float32)], 10)
    with pytest.raises(ValueError, match="max_bins = 2"):
        frontend.pack_utterances([ok], 2)
    frontend.pack_utterances([np.zeros(1600, np.float32), np.zeros(321, np.float32)], 10)     # both limits are inside


# ---- encode_ragged's host path ---------------------------------------------------------------------------------------------
def test_bins_are_checked_on_the_host_and_device_tensors_are_not_read():
    import torch
    from lsm_speech_classifier_amd import frontend
    got = frontend.checked_ragged_bins([12, 3, 7, 0, 11, 4], 6, 12)
    assert got.dtype == np.int32 and got.tolist() == [12, 3, 7, 0, 11, 4]
    assert frontend.checked_ragged_bins(np.array([0, 3], dtype=np.int64), 2, 3).tolist() == [0, 3]
    assert frontend.checked_ragged_bins(torch.tensor([5, 0], dtype=torch.int32), 2, 6).tolist() == [5, 0]
    for bad, n, tb, what in (([1, 5], 2, 12, r"bins \[1\] of clips \[0\]"), ([5, 2], 2, 12, r"bins \[2\] of clips \[1\]"),
                             ([-1, 5, 13], 3, 12, r"bins \[-1, 13\] of clips \[0, 2\]"), ([5], 2, 12, "must be 2 integers"),
                             ([5.0, 6.0], 2, 12, "must be 2 integers"), ([[5, 6]], 2, 12, "must be 2 integers")):
        with pytest.raises(ValueError, match=what):
            frontend.checked_ragged_bins(bad, n, tb)
    with pytest.raises(ValueError, match="int32"):
        frontend.checked_ragged_bins(torch.tensor([5, 0], dtype=torch.int64), 2, 6)
    with pytest.raises(ValueError, match="int32"):
        frontend.checked_ragged_bins(torch.tensor([5, 0, 3], dtype=torch.int32), 2, 6)


def test_a_front_end_of_another_shape_is_refused_with_the_reason():
    from lsm_speech_classifier_amd import frontend
    assert frontend.ragged_refusal(16000, 100) is None and frontend.ragged_refusal(480, 3) is None
    assert "n_samples = 16000" in frontend.ragged_refusal(16001, 100)
    assert "160 samples per time bin" in frontend.ragged_refusal(16000, 50)
    assert "time_bins >= 3" in frontend.ragged_refusal(320, 2)
    # the claim the definition rests on: gtgram on 160 * T samples at T bins has nwin 400, hop 160 and T - 2 columns, and
    # the mel hop max(1, int(L / T)) is 160
    for T in range(3, 700):
        L = 160 * T
        assert frontend.gtgram_strides(16000, 0.025, L / (16000 * T), L) == (400, 160, T - 2), T
        assert max(1, int(L / T)) == 160


def test_encode_ragged_refuses_on_the_host_before_any_launch():
    """A front end object made without a GPU (``__new__``): every refusal below is raised by host checks alone."""
    from lsm_speech_classifier_amd import frontend
    fe = frontend.SpikeFrontEnd.__new__(frontend.SpikeFrontEnd)
    fe.n_filters, fe.filterbank, fe.redundancy, fe.thresholds, fe.gap = 8, "gammatone", 1, [0.7], 0.1
    fe.time_bins, fe.n_samples, fe.device = 12, 16000, "cpu"
    with pytest.raises(ValueError, match="n_samples = 1920"):
        fe.encode_ragged(np.zeros((2, 16000), np.float32), [3, 4])
    fe.n_samples = 1920
    with pytest.raises(ValueError, match="clips must have 1920 samples"):
        fe.encode_ragged(np.zeros((2, 1000), np.float32), [3, 4])


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_four_functions_and_the_table_mirrors_them():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_ragged.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(NAMES)
    assert _lib.RAGGED_SYMBOLS == tuple(_lib.RAGGED_SIGS) and set(_lib.RAGGED_SYMBOLS) == set(NAMES)
    for name in NAMES:
        params = _params(header, name)
        res, args = _lib.RAGGED_SIGS[name]
        assert res is _lib.c_int and len(args) == len(params), name
        for p, ctype in zip(params, args):
            if "*" in p:
                assert ctype is _lib.c_void, f"{name}: {p}"
            elif p.startswith("float "):
                assert ctype is _lib.c_float, f"{name}: {p}"
            elif p.startswith("long "):
                assert ctype is _lib.C.c_long, f"{name}: {p}"
            else:
                assert p.startswith("int ") and ctype is _lib.c_int, f"{name}: {p}"
    base = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    # each spike encoder is its twin's list with the count arrays after time_bins (and clip_steps_out after the raster)
    for suffix, t in (("f64", "double"), ("f32", "float")):
        twin = _params(base, "lsm_spec_to_spikes_" + suffix)
        assert _params(header, "lsm_spec_to_spikes_ragged_" + suffix) == \
            twin[:5] + ["const int32_t *clip_cols", "const int32_t *clip_bins"] + twin[5:]
    twin = _params(base, "lsm_gammatone_spikes_f64")
    assert _params(header, "lsm_gammatone_spikes_ragged_f64") == \
        twin[:9] + ["const int32_t *clip_bins"] + twin[9:14] + ["int32_t *clip_steps_out"] + twin[14:]
    assert "NOT offered" in header and "lsm_hip_mask.h" in header                   # masks: said in the header


def test_the_new_table_is_disjoint_from_the_other_ten_and_the_exports_count_67():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
              _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS)
    for table in others:
        assert not set(NAMES) & set(table)
    assert sum(len(t) for t in others) == 63 and sum(len(t) for t in others) + len(_lib.RAGGED_SIGS) == 67
    for name in NAMES:                                              # no other header declares them
        for h in os.listdir(os.path.join(ROOT, "include")):
            declared = re.findall(_DECLARED, open(os.path.join(ROOT, "include", h)).read(), re.M)
            assert (name in declared) == (h == "lsm_hip_ragged.h"), (name, h)


def test_the_build_id_covers_the_new_header_and_source(tmp_path):
    from lsm_speech_classifier_amd import build
    assert "lsm_hip_ragged.h" in build.ABI_HEADERS and "ragged_frontend.hip" in build.SOURCES
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    text = (inc / "lsm_hip_ragged.h").read_bytes()
    (inc / "lsm_hip_ragged.h").write_bytes(text.replace(b"clip_bins", b"clip_bons", 1))
    assert build.source_id(str(inc)) != build.source_id()


def test_the_library_exports_the_four_names():
    from lsm_speech_classifier_amd import _lib, build
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NAMES:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name


# ---- the scripts' flags and File 1 -----------------------------------------------------------------------------------------
def test_variable_length_flags_parse_forward_and_change_nothing_without_them(monkeypatch):
    import argparse
    import create_dataset as cd
    import main as pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--resample", default="host")
    for add in (cd.add_augment_flags, cd.add_reverb_flags, cd.add_speed_flags, cd.add_mask_flags, cd.add_variable_length_flags):
        add(ap)
    none = ap.parse_args([])
    assert none.variable_length is False and none.max_seconds == 1.0
    a = ap.parse_args(["--variable-length", "--max-seconds", "0.75"])
    cd.check_variable_length_args(a)
    assert cd.max_bins_of(a.max_seconds) == 75 and cd.max_bins_of(1.0) == 100
    for bad in (["--variable-length", "--packed"], ["--variable-length", "--time-masks", "1", "--time-mask-width", "5"],
                ["--variable-length", "--rir-dir", "synthetic"], ["--variable-length", "--max-seconds", "0.02"]):
        with pytest.raises(SystemExit):
            cd.check_variable_length_args(ap.parse_args(bad))
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert calls[0][6:] == []
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, max_seconds=0.5)
    assert calls[0][6:] == ["--variable-length", "--max-seconds", "0.5"]
    with pytest.raises(SystemExit):
        pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, variable_length=True)


def test_file_1_keeps_its_schema_and_gains_n_steps(tmp_path):
    from lsm_speech_classifier_amd import spikefile
    import extract_lsm_features as ex
    rng = np.random.default_rng(1)
    X = (rng.random((5, 3, 40)) < 0.3).astype(np.uint8)
    steps = np.array([40, 12, 0, 28, 16], dtype=np.int32)
    for b, t in enumerate(steps):
        X[b, :, t:] = 0
    y = np.arange(5, dtype=np.int32)
    f = str(tmp_path / "ragged.npz")
    spikefile.save(f, X_spikes=X, y_labels=y, n_steps=steps)
    with np.load(f) as data:
        assert sorted(data.files) == ["X_spikes", "n_steps", "y_labels"] and data["n_steps"].dtype == np.int32
    X2, y2 = spikefile.load(f)
    assert np.array_equal(X2, X) and np.array_equal(y2, y) and np.array_equal(spikefile.load_steps(f), steps)
    g = str(tmp_path / "plain.npz")
    spikefile.save(g, X_spikes=X, y_labels=y)
    with np.load(g) as data:
        assert sorted(data.files) == ["X_spikes", "y_labels"]                    # without the flag: the file as before
    assert spikefile.load_steps(g) is None
    with pytest.raises(ValueError):
        spikefile.save(f, X_spikes=X, y_labels=y, n_steps=steps + 30)
    # the critical weight sums per-clip shapes: views of the clips' own steps, not the padded rows
    views = ex.clip_views(X, steps)
    assert [v.shape for v in views] == [(3, int(t)) for t in steps]

    class P:
        small_world_graph_k, membrane_threshold, refractory_period = 10, 2.0, 2
    density = X.sum() / (3 * steps.sum())
    assert ex.calculate_theoretical_w_critico(P, views) == (2.0 - 2 * density * 2) / 5
    assert ex.calculate_theoretical_w_critico(P, X) != ex.calculate_theoretical_w_critico(P, views)
