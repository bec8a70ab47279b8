"""Augmentation on ragged launches (SPEC.md 1.16, include/lsm_hip_ragged_augment.h), what can be checked without a GPU: the
header, the binding and the build lists, the refusals (made on the host before any launch, so fake aligned addresses serve),
`frontend.mask_plan_ragged` against `mask_plan` and against the draws restated from the text, the restatement of the ragged
mixer against the unragged one, and the flags of create_dataset.py and main.py."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402
import mix_restatement as MX  # noqa: E402
import ragged_augment_restatement as RA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lsm_mix_ragged_f32", "lsm_gammatone_spikes_ragged_masked_f64", "lsm_spec_to_spikes_ragged_masked_f64",
       "lsm_spec_to_spikes_ragged_masked_f32", "lsm_step_fused_ragged_masked_supported", "lsm_step_fused_ragged_masked_f64")


# ---- header, binding, build ---------------------------------------------------------------------------------------------
def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_binding_and_library_carry_the_six_names():
    from lsm_speech_classifier_amd import _lib, build
    header = _header("lsm_hip_ragged_augment.h")
    assert _lib.RAGGED_AUGMENT_SYMBOLS == tuple(_lib.RAGGED_AUGMENT_SIGS) == NEW
    for name in NEW:
        res, args = _lib.RAGGED_AUGMENT_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params), name
        for p, ctype in zip(params, args):
            want = _lib.c_void if "*" in p else C.c_long if p.startswith("long ") else _lib.c_int
            assert ctype is want, f"{name}: {p}"
    # each list is its twin's with the new parameters where the header says
    twin = _params(_header("lsm_hip_mix.h"), "lsm_mix_f32")
    assert _params(header, "lsm_mix_ragged_f32") == twin[:3] + ["const int32_t *clip_samples"] + twin[3:]
    masks = ["const uint32_t *freq_mask", "const uint32_t *time_mask"]
    for name, twin_header in (("lsm_gammatone_spikes_ragged", "lsm_hip_ragged.h"), ("lsm_spec_to_spikes_ragged", "lsm_hip_ragged.h"),
                              ("lsm_step_fused_ragged", "lsm_hip_step.h")):
        for suffix in ("_f64", "_f32") if "spec" in name else ("_f64",):
            twin = _params(_header(twin_header), name + suffix)
            assert _params(header, name + "_masked" + suffix) == twin[:-1] + masks + twin[-1:], name
    assert _params(header, "lsm_step_fused_ragged_masked_supported") == _params(_header("lsm_hip_step.h"), "lsm_step_fused_supported")
    # fifteen tables, disjoint, 83 exports; the fourteen older ones keep their sizes
    old = [_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
           _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS, _lib.RAGGED_SIGS, _lib.STEP_SIGS,
           _lib.STEP_STATE_SIGS, _lib.TRIM_SIGS]
    assert sum(len(t) for t in old) == 77 and len(set().union(*old)) == 77
    tables = old + [_lib.RAGGED_AUGMENT_SIGS]
    assert sum(len(t) for t in tables) == 83 and len(set().union(*tables)) == 83
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name
    assert "ragged_masked_frontend.hip" in build.SOURCES and "step_fused_ragged_masked.hip" in build.SOURCES
    assert "lsm_hip_ragged_augment.h" in build.ABI_HEADERS
    hashed = build.PUBLIC_HEADERS + build.ABI_HEADERS               # listed once, and not among the nine
    assert hashed.count("lsm_hip_ragged_augment.h") == 1 and "lsm_hip_ragged_augment.h" not in build.PUBLIC_HEADERS
    assert len(build.PUBLIC_HEADERS) == 9 and len(hashed) == 18         # nine, and the nine single-header lists before it
    with pytest.raises(OSError):                                    # the header is hashed into the build id
        build.source_id(include_dir=os.path.join(ROOT, "lsm-speech-classifier_amd"))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _in_order(call, later, texts):
    """Row `at` breaks its own rule AND every later one: the message names the earliest."""
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)


def test_the_ragged_mixers_refusals_in_their_order():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    A, N, O, L = 0x10000, 0x20000, 0x30000, 0x40000
    I = [0x50000 + 0x1000 * i for i in range(7)]                   # noise_row, noise_offset, shift, scale, ratio, gain, power
    good = dict(audio=A, n_clips=2, n_samples=1001, clip_samples=L, noise=N, M=3, noise_len=37, noise_row=I[0], noise_offset=I[1],
                shift=I[2], scale=I[3], ratio=I[4], out=O, gain_out=I[5], power_out=I[6])

    def call(fn=lib.lsm_mix_ragged_f32, **kw):
        a = dict(good, **kw)
        if fn is lib.lsm_mix_f32:
            del a["clip_samples"]
        counts = ("n_clips", "n_samples", "M", "noise_len")
        rc = fn(*[v if k in counts else (v or None) for k, v in a.items()], None)      # an address of 0 is NULL
        return rc, lib.lsm_last_error().decode()

    later = [dict(n_samples=0), dict(n_clips=-1), dict(noise_len=0), dict(M=0), dict(audio=A + 2), dict(noise=N + 1), dict(out=O + 2),
             dict(noise_row=I[0] + 2), dict(noise_offset=I[1] + 1), dict(shift=I[2] + 3), dict(scale=I[3] + 2), dict(ratio=I[4] + 4),
             dict(gain_out=I[5] + 4), dict(power_out=I[6] + 4), dict(clip_samples=0)]
    texts = ["n_samples=0", "negative number of rows", "noise_len=0", "n_noise_rows=0", "audio is misaligned", "noise is misaligned",
             "out is misaligned", "noise_row is misaligned", "noise_offset is misaligned", "shift is misaligned",
             "scale is misaligned", "ratio is misaligned", "gain_out is misaligned", "power_out is misaligned", "null clip_samples"]
    _in_order(call, later, texts)
    # the twin refuses the same calls with the same words, up to the ragged form's own
    for kw, text in zip(later[:-1], texts[:-1]):
        (rc, msg), (rc2, msg2) = call(**kw), call(lib.lsm_mix_f32, **kw)
        assert rc == rc2 == -1 and msg == msg2 and text in msg
    # a NULL buffer and out == audio come before the count array; NULL before misaligned
    for kw, text in ((dict(audio=0, clip_samples=0), "null buffer"), (dict(ratio=0, clip_samples=0), "null buffer"),
                     (dict(out=A, clip_samples=0), "must not be audio"), (dict(out=A, clip_samples=L + 2), "must not be audio"),
                     (dict(clip_samples=0), "null clip_samples"), (dict(clip_samples=L + 2), "clip_samples is misaligned"),
                     (dict(clip_samples=L + 1), "clip_samples is misaligned"), (dict(n_samples=(1 << 24) + 1), "n_samples=")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert call(n_clips=0)[0] == 0 and call(n_clips=0, clip_samples=0)[0] == 0       # nothing to do, nothing launched


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_the_masked_ragged_encoders_refusals_in_their_order(suffix):
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    dt = np.float64 if suffix == "f64" else np.float32
    on, off = np.array([0.9, 0.7], dtype=dt), np.array([0.8, 0.6], dtype=dt)
    D, Cc, B, R, Fm, Tm = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    good = dict(db=D, n_clips=2, F=5, ncols=38, tb=40, cols=Cc, bins=B, floor=1, n_thr=2, red=1, raster=R, norm=0, fm=Fm, tm=Tm)

    def call(name="lsm_spec_to_spikes_ragged_masked_" + suffix, **kw):
        a = dict(good, **kw)
        p = lambda v: v or None                                                    # noqa: E731
        args = [p(a["db"]), a["n_clips"], a["F"], a["ncols"], a["tb"], p(a["cols"]), p(a["bins"]), a["floor"], on.ctypes.data,
                off.ctypes.data, a["n_thr"], a["red"], p(a["raster"]), p(a["norm"])]
        if "masked" in name:
            args += [p(a["fm"]), p(a["tm"])]
        rc = getattr(lib, name)(*args, None)
        return rc, lib.lsm_last_error().decode()

    later = [dict(ncols=1), dict(db=0), dict(n_thr=9), dict(red=0), dict(cols=0), dict(bins=B + 2), dict(tb=2), dict(fm=Fm + 2)]
    texts = ["bad shape", "null input", "n_thr=9", "redundancy", "null per-clip count array", "4-byte aligned", "at least 3 time bins",
             "freq_mask and time_mask must be 4-byte aligned"]
    _in_order(call, later, texts)
    # the ragged twin gives the same answers up to the masks' own refusal
    for kw in later[:-1]:
        assert call(**kw) == call("lsm_spec_to_spikes_ragged_" + suffix, **kw)
    for kw in (dict(fm=Fm + 1), dict(tm=Tm + 2), dict(fm=0, tm=Tm + 3), dict(fm=Fm + 2, tm=0)):
        rc, msg = call(**kw)
        assert rc == -1 and "freq_mask and time_mask must be 4-byte aligned" in msg, (kw, rc, msg)
    assert call(n_clips=0, db=0, fm=Fm + 2)[0] == 0                 # an empty batch is accepted before its buffers, as the twin's


def test_the_masked_ragged_gammatone_refusals_in_their_order():
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    on, off = np.array([0.9, 0.7]), np.array([0.8, 0.6])
    A, K, B, R, S, W, Fm, Tm = (0x10000 * i for i in range(1, 9))
    F, tb = 8, 12
    ws_bytes = int(lib.lsm_gammatone_spikes_workspace(2, F, tb - 2))
    good = dict(audio=A, n_clips=2, n_samples=160 * tb, coefs=K, F=F, nwin=400, hop=160, ncols=tb - 2, tb=tb, bins=B, n_thr=2, red=1,
                raster=R, steps=S, ws=W, ws_bytes=ws_bytes, coef_flags=7, flags=0, fm=Fm, tm=Tm)

    def call(name="lsm_gammatone_spikes_ragged_masked_f64", **kw):
        a = dict(good, **kw)
        p = lambda v: v or None                                                    # noqa: E731
        args = [p(a["audio"]), a["n_clips"], a["n_samples"], p(a["coefs"]), a["F"], a["nwin"], a["hop"], a["ncols"], a["tb"],
                p(a["bins"]), on.ctypes.data, off.ctypes.data, a["n_thr"], a["red"], p(a["raster"]), p(a["steps"]), p(a["ws"]),
                a["ws_bytes"], a["coef_flags"], a["flags"]]
        if "masked" in name:
            args += [p(a["fm"]), p(a["tm"])]
        rc = getattr(lib, name)(*args, None)
        return rc, lib.lsm_last_error().decode()

    later = [dict(flags=4), dict(F=1), dict(nwin=0), dict(n_thr=9), dict(red=0), dict(audio=0), dict(ws_bytes=8), dict(ws=W + 4),
             dict(bins=0), dict(steps=S + 2), dict(tm=Tm + 2)]
    texts = ["launch_flags", "n_filters >= 2", "bad window", "n_thr=9", "redundancy", "null buffer", "workspace of 8 bytes",
             "workspace must be 8-byte aligned", "null per-clip count array", "clip_steps_out", "freq_mask and time_mask"]
    _in_order(call, later, texts)
    for kw in later[:-1]:
        assert call(**kw) == call("lsm_gammatone_spikes_ragged_f64", **kw)
    for kw, text in ((dict(bins=B + 2), "4-byte aligned"), (dict(n_samples=160 * tb - 1, ncols=tb - 3), "hop * time_bins"),
                     (dict(n_samples=160 * tb - 1, ncols=tb - 3, fm=Fm + 1), "hop * time_bins"), (dict(fm=Fm + 1), "freq_mask")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    rc, msg = call(F=1025, ws_bytes=1 << 40, fm=Fm + 1)             # the twin's LSM_ERR_UNSUPPORTED comes first too
    assert rc == -4 and "waves per clip" in msg
    assert frontend.RAGGED_HOP == 160


# ---- mask_plan_ragged ---------------------------------------------------------------------------------------------------
KW = dict(freq_masks=2, freq_width=9, time_masks=3, time_width=12, prob=0.8, seed=7)


def test_mask_plan_ragged_equals_mask_plan_at_full_length():
    from lsm_speech_classifier_amd import frontend
    for n, F, tb, kw in ((37, 33, 40, KW), (5, 128, 100, dict(time_masks=1, time_width=100)), (0, 16, 12, KW),
                         (9, 8, 12, dict(freq_masks=1, freq_width=8, prob=0.0))):
        full = frontend.mask_plan(n, F, tb, **kw)
        ragged = frontend.mask_plan_ragged(np.full(n, tb), F, tb, **kw)
        assert isinstance(ragged, frontend.MaskPlan)
        assert ragged.freq.dtype == ragged.time.dtype == np.uint32
        assert ragged.freq.shape == full.freq.shape and ragged.time.shape == full.time.shape == (n, (tb + 31) // 32)
        assert ragged.freq.tobytes() == full.freq.tobytes() and ragged.time.tobytes() == full.time.tobytes()
    assert frontend.mask_plan(37, 33, 40, **KW).time.any()


def test_mask_plan_ragged_keeps_every_band_inside_the_clip():
    from lsm_speech_classifier_amd import frontend
    bins = np.tile([0, 3, 5, 33, 40], 40)
    tb, F = 40, 33
    kw = dict(KW, time_width=40, prob=1.0)
    plan = frontend.mask_plan_ragged(bins, F, tb, **kw)
    assert plan.time.shape == (len(bins), 2) and plan.freq.shape == (len(bins), 2)
    fm, tm, (tp, tw) = RA.ragged_time_bands(bins, tb, kw["time_masks"], kw["time_width"], kw["freq_masks"], kw["freq_width"], F,
                                            kw["prob"], kw["seed"])
    assert np.array_equal(MR.bits_of(plan.time, tb), tm) and np.array_equal(MR.bits_of(plan.freq, F), fm)
    assert (tp >= 0).all() and (tp + tw <= bins[:, None]).all() and (tw <= bins[:, None]).all()
    bits = MR.bits_of(plan.time, 64)                                # the words' every bit, not only the first time_bins
    for b, T in enumerate(bins):
        assert not bits[b, T:].any(), f"clip {b} of {T} bins has a time bit at or behind its end"
    assert not bits[bins == 0].any() and bits[bins == 3].any() and bits[bins == 33][:, 32].any()
    # a width drawn wider than the clip is cut to the clip, so a short clip can be masked whole; the frequency words are
    # those of mask_plan (the draws are the same and in the same order)
    assert (tw[bins == 3] == 3).any() and bits[bins == 3][:, :3].all(axis=1).any()
    assert plan.freq.tobytes() == frontend.mask_plan(len(bins), F, tb, **kw).freq.tobytes()
    # prob: the fifth draw decides as it does in mask_plan, whose frequency words these are
    half = frontend.mask_plan_ragged(bins, F, tb, **dict(kw, prob=0.5))
    fm5, tm5, _ = RA.ragged_time_bands(bins, tb, kw["time_masks"], kw["time_width"], kw["freq_masks"], kw["freq_width"], F, 0.5,
                                       kw["seed"])
    assert np.array_equal(MR.bits_of(half.time, tb), tm5) and np.array_equal(MR.bits_of(half.freq, F), fm5)
    assert half.freq.tobytes() == frontend.mask_plan(len(bins), F, tb, **dict(kw, prob=0.5)).freq.tobytes()
    cleared = fm.any(axis=1) & ~fm5.any(axis=1)
    assert 0 < cleared.sum() < len(bins) and not tm5[cleared].any() and tm[cleared].any()


def test_mask_plan_ragged_refuses_what_mask_plan_refuses():
    from lsm_speech_classifier_amd import frontend
    bins = np.array([5, 12, 0])
    for bad in (dict(freq_masks=-1), dict(time_width=13), dict(freq_width=9), dict(prob=1.5), dict(time_masks=-2)):
        kw = dict(dict(freq_masks=1, freq_width=2, time_masks=1, time_width=2), **bad)
        with pytest.raises(ValueError) as full:
            frontend.mask_plan(3, 8, 12, **kw)
        with pytest.raises(ValueError) as ragged:
            frontend.mask_plan_ragged(bins, 8, 12, **kw)
        assert str(full.value) == str(ragged.value)
    for bad_bins in ([5, 13], [-1, 4], [[3, 4]], [3.5, 4.0]):
        with pytest.raises(ValueError, match="bins must be"):
            frontend.mask_plan_ragged(np.array(bad_bins), 8, 12, time_masks=1, time_width=2)


# ---- the mixer's restatement --------------------------------------------------------------------------------------------
def test_the_ragged_mix_restatement_is_the_clip_alone_and_ignores_the_tail():
    rng = np.random.default_rng(3)
    n, lengths = 700, [-3, 0, 1, 255, 256, 257, 700, 900]
    audio = rng.standard_normal((8, n)).astype(np.float32)
    noise = rng.standard_normal((2, 37)).astype(np.float32)
    args = (noise, np.full(8, 0.1), np.arange(8) % 2, np.arange(8) * 5, np.array([0, 5, -5, 3, -256, 2000, -2000, 0]),
            np.full(8, 0.5, np.float32))
    y, g, p = RA.mix_ragged(audio, lengths, *args)
    dirty = audio.copy()
    for b, m in enumerate(RA.clamp_samples(lengths, n)):
        dirty[b, m:] = np.nan
    y2, g2, p2 = RA.mix_ragged(dirty, lengths, *args)
    assert y.tobytes() == y2.tobytes() and g.tobytes() == g2.tobytes() and p.tobytes() == p2.tobytes()
    assert not y[0].any() and not y[1].any() and g[0] == g[1] == 0 and not p[:2].any() and not y[3, 255:].any() and y[3, :255].any()
    full = MX.mix(audio[6:], noise, *[a[6:] for a in args[1:]])
    assert y[6:].tobytes() == full[0].tobytes() and g[6:].tobytes() == full[1].tobytes()      # full length: the unragged form


# ---- the scripts' flags ---------------------------------------------------------------------------------------------------
def _parser(cd):
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--resample", default="host")
    for add in (cd.add_augment_flags, cd.add_reverb_flags, cd.add_speed_flags, cd.add_mask_flags, cd.add_variable_length_flags):
        add(ap)
    return ap


CHAIN_FLAGS = {"the corruption flags": ["--noise-dir", "synthetic", "--snr-db", "5,15"], "--rir-dir": ["--rir-dir", "synthetic"],
               "the mask flags": ["--time-masks", "1", "--time-mask-width", "5"]}


def test_the_new_flag_lets_the_chain_through_and_nothing_else(monkeypatch):
    import create_dataset as cd
    import main as pipeline
    ap = _parser(cd)
    assert ap.parse_args([]).augment_variable_length is False
    assert ap.parse_args(["--variable-length", "--augment-variable-length"]).augment_variable_length is True
    every = sum(CHAIN_FLAGS.values(), [])
    for name, flags in CHAIN_FLAGS.items():
        with pytest.raises(SystemExit) as e:                        # without the flag: today's refusal, word for word
            cd.check_variable_length_args(ap.parse_args(["--variable-length"] + flags))
        assert str(e.value) == f"--variable-length does not combine with {name}"
        cd.check_variable_length_args(ap.parse_args(["--variable-length", "--augment-variable-length"] + flags))
    with pytest.raises(SystemExit) as e:
        cd.check_variable_length_args(ap.parse_args(["--variable-length"] + every))
    assert str(e.value) == "--variable-length does not combine with the corruption flags, --rir-dir, the mask flags"
    a = ap.parse_args(["--variable-length", "--augment-variable-length", "--trim-silence", "30"] + every)
    cd.check_variable_length_args(a)
    assert cd.augment_from_args(a)["snr_db"] == (5.0, 15.0) and cd.reverb_from_args(a)["rir_dir"] == "synthetic"
    assert cd.mask_from_args(a)["time_width"] == 5 and cd.trim_from_args(a)["top_db"] == 30.0
    # what stays refused with the flag
    for flags, text in ((["--speed-factors", "0.9,1.1"], "--speed-factors"), (["--packed"], "--packed"),
                        (["--resample", "device"], "--resample device")):
        with pytest.raises(SystemExit, match="--variable-length does not combine with " + text):
            cd.check_variable_length_args(ap.parse_args(["--variable-length", "--augment-variable-length"] + flags + every))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--variable-length runs in one process"):
        cd.check_variable_length_args(ap.parse_args(["--variable-length", "--augment-variable-length"]))
    monkeypatch.delenv("WORLD_SIZE")
    # main.py forwards the flag with --variable-length, and nothing new without it
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, *k, **kw: calls.append(cmd) or 0)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, max_seconds=0.5)
    assert calls[0][6:] == ["--variable-length", "--max-seconds", "0.5"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, augment_variable_length=True, trim_silence=30.0,
                          time_masks=1, time_mask_width=5)
    assert calls[0][-10:] == ["--variable-length", "--max-seconds", "1.0", "--augment-variable-length", "--trim-silence", "30.0",
                             "--trim-pad-ms", "30.0", "--trim-min-ms", "30.0"]
    assert "--time-masks" in calls[0]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, augment_variable_length=True)
    assert "--augment-variable-length" not in calls[0] and "--variable-length" not in calls[0]


def test_the_builder_and_the_pipeline_take_the_chain():
    import inspect
    import create_dataset as cd
    from lsm_speech_classifier_amd import augment, frontend, pipeline
    sig = inspect.signature(cd.create_variable_length_dataset).parameters
    assert [sig[k].default for k in ("augment", "reverb", "mask")] == [None, None, None]
    sig = inspect.signature(pipeline.features_from_utterances).parameters
    assert [sig[k].default for k in ("corrupt", "reverb", "mask")] == [None, None, None]
    assert list(inspect.signature(frontend.NoiseMixer.mix_ragged).parameters) == [
        "self", "x", "lengths", "snr_db", "rows", "offsets", "shift", "scale", "out"]
    assert list(inspect.signature(frontend.mask_plan_ragged).parameters) == [
        "bins", "n_filters", "time_bins", "freq_masks", "freq_width", "time_masks", "time_width", "prob", "seed"]
    assert inspect.signature(frontend.SpikeFrontEnd.encode_ragged).parameters["mask"].default is None
    assert inspect.signature(pipeline.step_fused_ragged).parameters["mask"].default is None
    assert pipeline.STEP_FORMS == {"plain": 0, "masked": 1, "ragged": 2}
    # a ragged chain has no speed stage
    with pytest.raises(ValueError, match="speed perturbation is not offered"):
        augment.AugmentChain(speed=object()).apply_ragged(None, None, augment.StepPlans(speed=frontend.SpeedPlan(np.zeros(1, np.int32))))
