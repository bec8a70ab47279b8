"""Masks inside the spike encoders (SPEC.md 1.13): what can be checked without a GPU -- the new public header, its ctypes
table and the library's exports, the build id's cover of the header, the plan (`frontend.mask_plan`, `MaskPlan`,
`mask_words`) against the restatement of its draws (tests/mask_restatement.py), the restated definition on the case that
separates it from zeroing a raster, and the scripts' flags."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mask_restatement as MR  # noqa: E402

TWINS = {"lsm_spec_to_spikes_masked_f64": "lsm_spec_to_spikes_f64", "lsm_spec_to_spikes_masked_f32": "lsm_spec_to_spikes_f32",
         "lsm_gammatone_spikes_masked_f64": "lsm_gammatone_spikes_f64", "lsm_mel_spikes_masked_f32": "lsm_mel_spikes_f32"}
_DECLARED = r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\("


def _params(header: str, name: str):
    proto = re.search(r"^int\s+%s\((.*?)\);" % name, header, re.S | re.M).group(1)
    return [" ".join(p.split()) for p in proto.split(",")]


# ---- header, ctypes table, library -----------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_four_functions_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip_mask.h")).read()
    base = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    assert '#include "lsm_hip.h"' in header
    assert sorted(re.findall(_DECLARED, header, re.M)) == sorted(TWINS)
    assert _lib.MASK_SYMBOLS == tuple(_lib.MASK_SIGS) and set(_lib.MASK_SYMBOLS) == set(TWINS)
    for name, twin in TWINS.items():
        params, twin_params = _params(header, name), _params(base, twin)
        # the twin's list with the two mask pointers inserted before the stream
        assert params == twin_params[:-1] + ["const uint32_t *freq_mask", "const uint32_t *time_mask"] + twin_params[-1:], name
        res, args = _lib.MASK_SIGS[name]
        assert res is _lib.c_int and len(args) == len(params)
        for p, ctype, twin_ctype in zip(params, args, _lib._SIGS[twin][1] + [None, None]):
            if "*" in p:
                assert ctype is _lib.c_void, f"{name}: {p}"
            elif p.startswith("float "):
                assert ctype is _lib.c_float, f"{name}: {p}"
            elif p.startswith("long "):
                assert ctype is _lib.C.c_long, f"{name}: {p}"
            else:
                assert p.startswith("int ") and ctype is _lib.c_int, f"{name}: {p}"
        assert args[:-3] == _lib._SIGS[twin][1][:-1] and args[-3:] == [_lib.c_void] * 3


def test_the_new_table_is_disjoint_from_the_other_nine_which_keep_their_counts():
    from lsm_speech_classifier_amd import _lib
    others = (_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
              _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS)
    for table in others:
        assert not set(TWINS) & set(table)
    assert len(_lib.EXPORTED_SYMBOLS) == len(_lib._SIGS) == 38
    assert sum(len(t) for t in others) == 59 and sum(len(t) for t in others) + len(_lib.MASK_SIGS) == 63
    for name in list(TWINS) + list(TWINS.values()):                 # no existing header gained a declaration
        for h in os.listdir(os.path.join(ROOT, "include")):
            declared = re.findall(_DECLARED, open(os.path.join(ROOT, "include", h)).read(), re.M)
            assert (name in declared) == (h == ("lsm_hip_mask.h" if name in TWINS else "lsm_hip.h")), (name, h)


def test_the_build_id_covers_the_new_header(tmp_path):
    from lsm_speech_classifier_amd import build
    assert len(build.PUBLIC_HEADERS) == 9 and "lsm_hip_mask.h" not in build.PUBLIC_HEADERS
    assert "lsm_hip_mask.h" in build.ABI_HEADERS and "mask.hip" in build.SOURCES
    assert {"gammatone_spikes_body.h", "gammatone_spikes_kernel.inc", "mel_spikes_kernel.inc"} <= set(build.HEADERS)
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    text = (inc / "lsm_hip_mask.h").read_bytes()
    (inc / "lsm_hip_mask.h").write_bytes(text.replace(b"freq_mask", b"freq_mosk", 1))
    assert build.source_id(str(inc)) != build.source_id()
    (inc / "lsm_hip_mask.h").write_bytes(text)
    assert build.source_id(str(inc)) == build.source_id()


def test_the_library_exports_the_four_names():
    from lsm_speech_classifier_amd import _lib, build
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in TWINS:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name


# ---- the plan --------------------------------------------------------------------------------------------------------------
ARGS = dict(freq_masks=2, freq_width=9, time_masks=3, time_width=25, prob=0.7, seed=11)


def test_the_plan_is_the_restated_draws_and_slices_like_the_other_plans():
    from lsm_speech_classifier_amd import frontend
    n, F, Tb = 60, 70, 100
    plan = frontend.mask_plan(n, F, Tb, **ARGS)
    again = frontend.mask_plan(n, F, Tb, **ARGS)
    assert isinstance(plan, frontend.MaskPlan) and plan.freq.dtype == plan.time.dtype == np.uint32
    assert plan.freq.shape == (n, 3) and plan.time.shape == (n, 4)
    assert np.array_equal(plan.freq, again.freq) and np.array_equal(plan.time, again.time)
    fm, tm, ((fp, fw), (tp, tw)) = MR.plan_bits(n, F, Tb, **ARGS)
    assert np.array_equal(MR.bits_of(plan.freq, F), fm) and np.array_equal(MR.bits_of(plan.time, Tb), tm)
    assert np.array_equal(plan.freq, MR.words_of(fm)) and np.array_equal(plan.time, MR.words_of(tm))      # no bit beyond
    # widths never exceed their parameter, bands stay inside their axis, some clips are left alone and some are not
    assert fw.max() <= 9 and tw.max() <= 25 and fw.min() == 0 and (fp >= 0).all() and (fp + fw <= F).all()
    assert (tp >= 0).all() and (tp + tw <= Tb).all()
    assert fm.sum(1).max() <= 18 and tm.sum(1).max() <= 75
    clear = ~fm.any(1) & ~tm.any(1)
    assert 5 < clear.sum() < 40
    another = frontend.mask_plan(n, F, Tb, **dict(ARGS, seed=12))
    assert not np.array_equal(another.time, plan.time)
    # part / take
    part = plan.part(10, 25)
    assert np.array_equal(part.freq, plan.freq[10:25]) and np.array_equal(part.time, plan.time[10:25])
    idx = [7, 3, 59, 3]
    take = plan.take(idx)
    assert np.array_equal(take.freq, plan.freq[idx]) and np.array_equal(take.time, plan.time[idx])
    # a listing's plan does not depend on who slices it: the first clips of a longer listing differ (the draws are made
    # array by array), the slices of one listing agree
    assert np.array_equal(plan.part(0, 30).time, frontend.mask_plan(n, F, Tb, **ARGS).time[:30])
    # prob = 0: all clear; no counts: all clear; zero clips
    none = frontend.mask_plan(n, F, Tb, **dict(ARGS, prob=0.0))
    assert not none.freq.any() and not none.time.any()
    empty = frontend.mask_plan(n, F, Tb)
    assert not empty.freq.any() and not empty.time.any() and empty.freq.shape == (n, 3)
    assert frontend.mask_plan(0, F, Tb, **ARGS).time.shape == (0, 4)
    full = frontend.mask_plan(4, 33, 64, freq_masks=1, freq_width=33, time_masks=1, time_width=64, seed=3)
    assert full.freq.shape == (4, 2) and full.time.shape == (4, 2)


def test_mask_words_builds_plans_by_hand():
    from lsm_speech_classifier_amd import frontend
    w = frontend.mask_words([[0, 63], [69, 5]], [[1, 2], [1, 0]], 70)
    assert w.dtype == np.uint32 and w.shape == (2, 3)
    assert w.tolist() == [[1, 1 << 31, 1], [0, 0, 1 << 5]]
    assert frontend.mask_words([[60]], [[11]], 100).tolist() == [[0, 0xF0000000, 0x7F, 0]]
    bits = MR.bits_of(frontend.mask_words([[31]], [[2]], 100), 100)
    assert np.flatnonzero(bits[0]).tolist() == [31, 32]
    for bad in (([[69]], [[2]], 70), ([[-1]], [[1]], 70), ([[0]], [[-1]], 70), ([[0.5]], [[1]], 70), ([0], [1], 70),
                ([[0]], [[1]], 0)):
        with pytest.raises(ValueError):
            frontend.mask_words(*bad)


def test_the_other_plans_draw_for_seed_42_what_they_always_did():
    from lsm_speech_classifier_amd import frontend
    frontend.mask_plan(50, 40, 100, **dict(ARGS, seed=42))
    mix = frontend.mix_plan(40, 3, 100, (0.0, 20.0), max_shift=10, level_db=(-6.0, 0.0), seed=42)
    ref = np.random.RandomState(42)
    assert np.array_equal(mix.rows, ref.randint(0, 3, size=40)) and np.array_equal(mix.offsets, ref.randint(0, 100, size=40))
    assert np.array_equal(mix.shift, ref.randint(-10, 11, size=40))
    assert np.array_equal(mix.snr_db, 0.0 + 20.0 * ref.random_sample(40))
    rs = np.random.RandomState([42, 1])
    rows = rs.randint(0, 5, size=200)
    assert np.array_equal(frontend.reverb_plan(200, 5, prob=0.7, seed=42).rows, np.where(rs.random_sample(200) >= 0.7, -1, rows))
    rs = np.random.RandomState([42, 2])
    choice = rs.randint(0, 4, size=200)
    assert np.array_equal(frontend.speed_plan(200, 4, prob=0.6, seed=42).choice, np.where(rs.random_sample(200) >= 0.6, -1, choice))


def test_the_plan_refuses_what_it_cannot_draw():
    from lsm_speech_classifier_amd import frontend
    for bad in (dict(freq_masks=1, freq_width=41), dict(time_masks=1, time_width=101), dict(freq_masks=-1, freq_width=3),
                dict(time_masks=-1), dict(freq_width=-1), dict(time_width=-2), dict(prob=1.5), dict(prob=-0.1)):
        with pytest.raises(ValueError):
            frontend.mask_plan(10, 40, 100, **bad)
    with pytest.raises(ValueError):
        frontend.mask_plan(-1, 40, 100)
    with pytest.raises(ValueError):
        frontend.mask_plan(3, 0, 100)
    plan = frontend.mask_plan(4, 40, 100, **ARGS)
    frontend.checked_mask(plan, 4, 40, 100)
    for bad, n, F, Tb in ((plan, 5, 40, 100), (plan, 4, 70, 100), (plan, 4, 40, 130), ((plan.freq, plan.time), 4, 40, 100),
                          (frontend.MaskPlan(plan.freq.astype(np.int32), plan.time), 4, 40, 100)):
        with pytest.raises(ValueError):
            frontend.checked_mask(bad, n, F, Tb)


# ---- the restated definition -----------------------------------------------------------------------------------------------
def test_a_mask_releases_the_latch_where_a_zeroed_raster_switches_it_on_again():
    """One row 0.75, 0.65, 0.65, ..., threshold 0.7 with gap 0.1, time bin 3 masked: the latch is on for bins 0-2, released
    by the masked bin and never set again (0.65 lies between the bounds); the unmasked raster with step 3 zeroed is on
    again from bin 4."""
    Tb = 12
    db = np.full((2, Tb), 0.65)
    db[0, 0] = 0.75
    db[1, :] = 0.0
    db[1, 1] = 1.0                                                  # fixes the clip's range: values stay what they are
    tm = np.arange(Tb) == 3
    S, raster = MR.masked_raster(db, Tb, False, [0.7], 0.1, 1, None, tm)
    plain_S, plain = MR.masked_raster(db, Tb, False, [0.7], 0.1, 1)
    assert abs(plain_S[0, 0] - 0.75) < 1e-7 and abs(plain_S[0, 5] - 0.65) < 1e-7 and S[0, 3] == 0.0 and plain_S[0, 3] != 0.0
    assert raster[0].tolist() == [1, 1, 1] + [0] * (Tb - 3)
    assert plain[0].tolist() == [1] * Tb
    zeroed = MR.zeroed_raster(plain, 1, 1, None, tm)
    assert zeroed[0].tolist() == [1, 1, 1, 0] + [1] * (Tb - 4)
    assert not np.array_equal(zeroed, raster)
    # a masked row is all zeros in both, with redundancy; a non-positive threshold compares the 0.0 like any value
    fm = np.array([True, False])
    _, r2 = MR.masked_raster(db, Tb, False, [0.7], 0.1, 2, fm, None)
    assert r2.shape == (4, Tb) and not r2[:2].any() and np.array_equal(r2[2:], np.repeat(plain[1:], 2, axis=0))
    _, neg = MR.masked_raster(db, Tb, False, [-0.5], 0.1, 1, None, tm)
    assert neg[0].tolist() == [1] * Tb                              # 0.0 > -0.5: the definition is the arithmetic
    # a NaN clip: every unmasked value NaN, every masked one 0.0, nothing above a positive threshold
    bad = db.copy()
    bad[1, 4] = np.nan
    Sn, rn = MR.masked_raster(bad, Tb, False, [0.7], 0.1, 1, None, tm)
    assert not rn.any() and np.isnan(Sn[:, 0]).all() and (Sn[:, 3] == 0.0).all()


def test_the_restatement_reads_the_word_layout_of_the_abi():
    bits = np.zeros((2, 70), dtype=bool)
    bits[0, [0, 31, 32, 63, 64, 69]] = True
    words = MR.words_of(bits)
    assert words.tolist() == [[0x80000001, 0x80000001, 0x21], [0, 0, 0]]
    assert np.array_equal(MR.bits_of(words, 70), bits)
    words[0, 2] |= np.uint32(1 << 6)                                # a set bit at F: ignored
    assert np.array_equal(MR.bits_of(words, 70), bits)


# ---- the scripts' flags ----------------------------------------------------------------------------------------------------
def test_mask_flags_parse_and_nothing_without_them():
    import argparse
    import inspect
    import create_dataset as cd
    ap = argparse.ArgumentParser()
    cd.add_augment_flags(ap)
    cd.add_mask_flags(ap)
    none = ap.parse_args([])
    assert cd.mask_from_args(none) is None and none.mask_prob == 1.0
    assert cd.mask_from_args(ap.parse_args(["--freq-masks", "2"])) is None           # a count without a width masks nothing
    assert cd.mask_from_args(ap.parse_args(["--time-mask-width", "20"])) is None
    a = ap.parse_args(["--freq-masks", "2", "--freq-mask-width", "8", "--time-masks", "1", "--time-mask-width", "20",
                       "--mask-prob", "0.5", "--augment-seed", "9"])
    mask = cd.mask_from_args(a)
    assert mask == dict(freq_masks=2, freq_width=8, time_masks=1, time_width=20, prob=0.5, seed=9)
    assert cd.augment_from_args(a) is None

    class FE:
        n_filters, time_bins = 40, 100
    plan = cd.masks(mask, 30, FE)
    want = cd._frontend().mask_plan(30, 40, 100, **mask)
    assert np.array_equal(plan.freq, want.freq) and np.array_equal(plan.time, want.time) and plan.time.any()
    for bad in (["--freq-masks", "-1"], ["--time-mask-width", "-3"], ["--mask-prob", "2", "--time-masks", "1"]):
        with pytest.raises(SystemExit):
            cd.mask_from_args(ap.parse_args(bad))
    with pytest.raises(SystemExit):                                 # wider than the axis: refused with the flags named
        cd.masks(dict(mask, freq_width=41), 30, FE)
    assert inspect.signature(cd.create_dataset).parameters["mask"].default is None


def test_the_stage_receives_the_plan_with_the_flags_and_none_without(monkeypatch):
    """create_dataset() on a tiny synthetic corpus with a front end that records its calls: without the flags `encode` is
    called without a mask keyword, with them every batch gets its slice of the listing's plan."""
    import create_dataset as cd
    import torch
    calls = []

    class FakeFE:
        n_filters, time_bins, n_channels, n_steps, device = 8, 100, 8, 400, "cpu"

        def __init__(self, *a, **k):
            pass

        def encode(self, batch, **kw):
            calls.append((len(batch), kw))
            return torch.zeros((len(batch), 8, 400), dtype=torch.uint8)

    class FakeFrontend:
        SpikeFrontEnd = FakeFE
        mask_plan = staticmethod(cd._frontend().mask_plan)
        pack_raster = staticmethod(lambda r: r)

    monkeypatch.setattr(cd, "_frontend", lambda: FakeFrontend)
    monkeypatch.setattr(cd, "_synthetic_audio", lambda commands, n: (np.zeros((len(commands) * n, 16000), np.float32),
                                                                      list(range(len(commands))) * n))
    monkeypatch.setattr(cd, "ENCODE_BATCH", 4)
    saved = {}
    from lsm_speech_classifier_amd import spikefile
    monkeypatch.setattr(spikefile, "save", lambda path, **kw: saved.update(kw))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    cd.create_dataset(8, "gammatone", commands=["a", "b", "c"], synthetic_per_class=2)
    assert [c[0] for c in calls] == [4, 2] and all(kw == {} for _, kw in calls)
    calls.clear()
    mask = dict(freq_masks=1, freq_width=3, time_masks=2, time_width=30, prob=1.0, seed=5)
    cd.create_dataset(8, "gammatone", commands=["a", "b", "c"], synthetic_per_class=2, mask=mask)
    plan = cd._frontend().mask_plan(6, 8, 100, **mask)
    assert [c[0] for c in calls] == [4, 2] and all(set(kw) == {"mask"} for _, kw in calls)
    got = [kw["mask"] for _, kw in calls]
    assert np.array_equal(got[0].time, plan.time[:4]) and np.array_equal(got[1].time, plan.time[4:])
    assert np.array_equal(got[0].freq, plan.freq[:4]) and np.array_equal(got[1].freq, plan.freq[4:]) and plan.time.any()


def test_main_forwards_the_mask_flags_to_stage_1_and_nothing_without_them(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert calls[0][1:] == [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, time_masks=2, time_mask_width=20, mask_prob=0.5, augment_seed=7)
    assert calls[0][6:] == ["--freq-masks", "0", "--freq-mask-width", "0", "--time-masks", "2", "--time-mask-width", "20",
                            "--mask-prob", "0.5", "--augment-seed", "7"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, freq_masks=2)            # a count without a width: nothing
    assert calls[0][6:] == []
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, speed_factors="1.1", freq_masks=1, freq_mask_width=8)
    assert calls[0][6:] == ["--speed-factors", "1.1", "--speed-prob", "1.0", "--augment-seed", "42", "--freq-masks", "1",
                            "--freq-mask-width", "8", "--time-masks", "0", "--time-mask-width", "0", "--mask-prob", "1.0"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, freq_masks=1, freq_mask_width=8)
    code = calls[0][2]
    assert "'freq_masks': 1" in code and "'freq_mask_width': 8" in code and "cd.mask_from_args(a)" in code
    compile(code, "<in-memory stage>", "exec")
    with pytest.raises(TypeError):
        pipeline.run_pipeline(128, "gammatone", "original", 0.6, mask_seed=1)
    out = __import__("subprocess").run([sys.executable, os.path.join(ROOT, "main.py"), "--help"], capture_output=True,
                                       text=True, timeout=300)
    for flag in ("--freq-masks", "--freq-mask-width", "--time-masks", "--time-mask-width", "--mask-prob"):
        assert flag in out.stdout
