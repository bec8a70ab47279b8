"""Speed perturbation on ragged batches (SPEC.md 1.18, include/lsm_hip_ragged_speed.h), what can be checked without a GPU: the
header, the binding and the build lists, `lsm_speed_ragged_length` (host only) against Python integers, the refusals (made on
the host before any launch, so fake aligned addresses serve), the restatement (tests/speed_ragged_restatement.py) against
`scipy.signal.resample_poly` of the clip alone, `frontend.speed_ragged_lengths`, `AugmentChain.speed_ragged` in front of
`apply_ragged`, and the flags of create_dataset.py and main.py."""
import argparse
import ctypes as C
import inspect
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import speed_ragged_restatement as SRR  # noqa: E402
import speed_restatement as SR  # noqa: E402

NEW = ("lsm_speed_ragged_length", "lsm_speed_ragged_f32")
DESIGNS = ["9/10", "11/10", "1/2", "2"]
INT_MAX = 2 ** 31 - 1


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _params(header, name):
    m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _host_perturber(factors):
    """A `frontend.SpeedPerturber` with what the host reads of it (factors, designs, row_of_choice) and no device."""
    from lsm_speech_classifier_amd import frontend
    sp = frontend.SpeedPerturber.__new__(frontend.SpeedPerturber)
    sp.factors = list(factors)
    sp.tables, sp.row_of_choice = frontend.speed_bank(sp.factors)
    offsets = np.cumsum([0] + [len(t.taps) for t in sp.tables])
    sp.designs = np.ascontiguousarray([[t.up, t.down, len(t.taps), t.delay, int(o)] for t, o in zip(sp.tables, offsets)],
                                      dtype=np.int32)
    return sp


# ---- header, binding, build ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_the_two_names():
    from lsm_speech_classifier_amd import _lib, build
    header = _header("lsm_hip_ragged_speed.h")
    assert '#include "lsm_hip.h"' in header
    assert re.findall(r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\(", header, re.M) == list(NEW)
    assert _lib.RAGGED_SPEED_SYMBOLS == tuple(_lib.RAGGED_SPEED_SIGS) == NEW
    for name in NEW:
        res, args = _lib.RAGGED_SPEED_SIGS[name]
        params = _params(header, name)
        assert res is _lib.c_int and len(args) == len(params), name
        for p, ctype in zip(params, args):
            assert ctype is (_lib.c_void if "*" in p else _lib.c_int), f"{name}: {p}"
    # the launch's list is its twin's with the new parameters where the header says
    twin = _params(_header("lsm_hip_speed.h"), "lsm_speed_f32")
    assert _params(header, "lsm_speed_ragged_f32") == twin[:4] + ["const int32_t *clip_samples"] + twin[4:-1] + [
        "int32_t *clip_samples_out", "int32_t *clip_bins_out", "int time_bins"] + twin[-1:]
    assert _params(header, "lsm_speed_ragged_length") == ["int n_b", "int up", "int down", "int n_out"]
    # a table of its own, disjoint from the eighteen before it, which keep their sizes
    old = [_lib._SIGS, _lib.STREAM_SIGS, _lib.AUDIO_SIGS, _lib.MEL_STREAM_SIGS, _lib.RESAMPLE_SIGS, _lib.ADAPTIVE_SIGS,
           _lib.MIX_SIGS, _lib.REVERB_SIGS, _lib.SPEED_SIGS, _lib.MASK_SIGS, _lib.RAGGED_SIGS, _lib.STEP_SIGS,
           _lib.STEP_STATE_SIGS, _lib.TRIM_SIGS, _lib.RAGGED_AUGMENT_SIGS, _lib.READOUT_SIGS, _lib.FIT_SIGS, _lib.ENDPOINT_SIGS]
    assert [len(t) for t in old] == [38, 2, 2, 3, 3, 3, 3, 3, 2, 4, 4, 5, 3, 2, 6, 3, 2, 3]
    assert not set(NEW) & set().union(*old) and set(_lib.SPEED_SIGS) == {"lsm_speed_lds_bytes", "lsm_speed_f32"}
    for name in NEW:                                                # no other header declares them
        for h in os.listdir(os.path.join(ROOT, "include")):
            assert (re.search(r"\b%s\s*\(" % name, _header(h)) is not None) == (h == "lsm_hip_ragged_speed.h"), (name, h)
    lib = _lib.load()                                               # loads without a GPU; rebuilds a stale library once
    blob = open(build.lib_path(), "rb").read()
    for name in NEW:
        assert hasattr(lib, name) and name.encode() + b"\0" in blob, name


def test_the_build_id_covers_the_new_header_and_the_older_lists_keep_their_sizes(tmp_path):
    from lsm_speech_classifier_amd import build
    assert build.RAGGED_SPEED_HEADERS == ["lsm_hip_ragged_speed.h"] and "speed.hip" in build.SOURCES
    assert len(build.PUBLIC_HEADERS) == 9 and len(build.ABI_HEADERS) == 9
    assert "lsm_hip_ragged_speed.h" not in build.PUBLIC_HEADERS + build.ABI_HEADERS
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(ROOT, "include"), inc)
    assert build.source_id(str(inc)) == build.source_id()
    text = (inc / "lsm_hip_ragged_speed.h").read_bytes()
    (inc / "lsm_hip_ragged_speed.h").write_bytes(text.replace(b"clip_samples", b"clip_somples", 1))
    assert build.source_id(str(inc)) != build.source_id()


# ---- the length formula -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", DESIGNS)
def test_the_length_export_is_ceil_in_python_integers(factor):
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    t = frontend.speed_design(factor)
    up, down = int(t.up), int(t.down)
    assert (up, down) == {"9/10": (10, 9), "11/10": (10, 11), "1/2": (2, 1), "2": (1, 2)}[factor]
    edge = 2 ** 31 // up                                            # n_b * up crosses 2^31 here
    lengths = [0, 1, 159, 160, 161, 1843, 1844, 2500] + [edge + d for d in (-2, -1, 0, 1, 2) if edge + d <= INT_MAX] + [
        INT_MAX // up, INT_MAX - 1, INT_MAX]
    for n_b in lengths:
        want = -(-n_b * up // down)
        for n_out in (2600, INT_MAX, 1, 0):
            got = int(lib.lsm_speed_ragged_length(n_b, up, down, n_out))
            assert got == min(want, n_out) == SRR.new_length(n_b, t, n_out), (n_b, n_out, got)
    assert int(lib.lsm_speed_ragged_length(1843, 10, 9, INT_MAX)) == 2048 and int(lib.lsm_speed_ragged_length(1844, 10, 9, INT_MAX)) == 2049
    assert int(lib.lsm_speed_ragged_length(-7, up, down, 100)) == 0                 # a count below 0 is 0, as in the kernel
    assert int(lib.lsm_speed_ragged_length(2500, 1, 1, 2600)) == 2500 and int(lib.lsm_speed_ragged_length(2700, 1, 1, 2600)) == 2600
    for bad in ((5, 0, 9, 10), (5, 10, 0, 10), (5, -1, 9, 10), (5, 10, 9, -1)):
        assert int(lib.lsm_speed_ragged_length(*bad)) == -1 and b"must be >= 1" in lib.lsm_last_error()


def test_speed_ragged_lengths_is_the_export_per_clip_of_a_plan():
    from lsm_speech_classifier_amd import frontend
    sp = _host_perturber(["9/10", 1, "11/10", "2"])
    lengths = np.array([480, 480, 480, 480, 6400, 6400, 0, -5, 5761], dtype=np.int64)
    choice = np.array([0, 1, 2, 3, 0, -1, 0, 2, 0], dtype=np.int32)
    got = frontend.speed_ragged_lengths(lengths, choice, sp, 6400)
    assert got.dtype == np.int64 and got.tolist() == [534, 480, 437, 240, 6400, 6400, 0, 0, 6400]
    tables = {0: sp.tables[0], 1: None, 2: sp.tables[1], 3: sp.tables[2], -1: None}
    assert got.tolist() == [SRR.new_length(max(n, 0), tables[c], 6400) for n, c in zip(lengths.tolist(), choice.tolist())]
    assert frontend.speed_ragged_lengths([1843, 1844], None, sp, 2600).tolist() == [2048, 2049]     # no choice: factor 0
    assert frontend.speed_ragged_lengths(np.zeros(0, np.int64), None, sp, 10).shape == (0,)
    assert list(inspect.signature(frontend.speed_ragged_lengths).parameters) == ["lengths", "choice", "perturber", "n_out"]
    assert list(inspect.signature(frontend.SpeedPerturber.perturb_ragged).parameters) == [
        "self", "audio", "lengths", "choice", "n_out", "time_bins", "out"]
    for bad in (dict(lengths=[1.5, 2.0]), dict(lengths=[[1, 2]]), dict(lengths=[2 ** 31]), dict(choice=[0]), dict(choice=[4, 0]),
                dict(n_out=-1), dict(n_out=2 ** 31)):
        with pytest.raises(ValueError):
            frontend.speed_ragged_lengths(**dict(dict(lengths=[5, 6], choice=[0, 1], perturber=sp, n_out=10), **bad))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_the_ragged_speed_launch_refuses_in_the_documented_order():
    from lsm_speech_classifier_amd import _lib, frontend
    lib = _lib.load()
    tables = [frontend.speed_design(f) for f in ("9/10", "11/10")]
    offsets = np.cumsum([0] + [len(t.taps) for t in tables])
    designs = np.ascontiguousarray([[t.up, t.down, len(t.taps), t.delay, int(o)] for t, o in zip(tables, offsets)], dtype=np.int32)
    A, T, O, L, R, S, Bn = (0x10000 * i for i in range(1, 8))
    good = dict(audio=A, fmt=0, n_clips=3, n_in=2500, clip_samples=L, taps=T, total=int(offsets[-1]), designs=designs, nd=2,
                design_row=R, n_out=2600, out=O, samples_out=S, bins_out=Bn, time_bins=16)

    def call(fn="lsm_speed_ragged_f32", **kw):
        a = dict(good, **kw)
        d = np.ascontiguousarray(a["designs"], dtype=np.int32)
        p = lambda v: v or None                                                    # noqa: E731  an address of 0 is NULL
        args = [p(a["audio"]), a["fmt"], a["n_clips"], a["n_in"]] + ([p(a["clip_samples"])] if "ragged" in fn else []) + [
            p(a["taps"]), a["total"], C.c_void_p(d.ctypes.data), a["nd"], p(a["design_row"]), a["n_out"], p(a["out"])]
        if "ragged" in fn:
            args += [p(a["samples_out"]), p(a["bins_out"]), a["time_bins"]]
        rc = getattr(lib, fn)(*args, None)
        return rc, lib.lsm_last_error().decode()

    # the twin's refusals, in its order, with its words -- and each ahead of every refusal of the ragged form's own
    own = dict(clip_samples=0, samples_out=S + 2, bins_out=Bn + 2, time_bins=2)
    big = np.array([[1000, 1001, 21022, 10, 0]], dtype=np.int32)
    twins = [dict(fmt=2), dict(nd=0), dict(total=0), dict(designs=[[10, 10, 209, 12, 0]], nd=1), dict(total=int(offsets[-1]) - 1),
             dict(audio=0), dict(taps=0), dict(audio=A + 2), dict(taps=T + 4), dict(design_row=R + 2), dict(n_clips=0),
             dict(n_clips=65536), dict(n_in=0), dict(n_out=0), dict(out=0), dict(out=O + 2), dict(out=A)]
    texts = ["sample_format=2", "n_designs=0 outside", "n_taps_total=0", "up == down", "runs past the n_taps_total", "null buffer",
             "null buffer", "audio is misaligned", "taps_dev is misaligned", "design_row is misaligned", "n_clips=0 outside",
             "n_clips=65536 outside", "n_in=0", "n_out=0", "out is required", "out is misaligned", "out must not be audio"]
    for kw, text in zip(twins, texts):
        (rc, msg), (rc2, msg2) = call(**dict(own, **kw)), call("lsm_speed_f32", **kw)
        assert rc == rc2 == -1 and msg == msg2 and text in msg, (kw, rc, msg, rc2, msg2)
    for at in range(len(twins) - 1):                                # the earlier of two twin refusals is named
        rc, msg = call(**dict(twins[at + 1], **twins[at]))
        assert rc == -1 and texts[at] in msg, (at, msg)
    (rc, msg), (rc2, msg2) = call(designs=big, nd=1, total=21022, **own), call("lsm_speed_f32", designs=big, nd=1, total=21022)
    assert rc == rc2 == -4 and msg == msg2 and "184000 bytes" in msg                # the twin's other code comes first too
    # the ragged form's own: row `at` breaks its rule AND every later one, the message names the earliest
    later = [dict(clip_samples=0), dict(clip_samples=L + 2), dict(samples_out=S + 2), dict(bins_out=Bn + 1), dict(time_bins=2),
             dict(n_out=2559)]
    words = ["null clip_samples", "clip_samples is misaligned", "clip_samples_out is misaligned", "clip_bins_out is misaligned",
             "time_bins=2", "n_out=2559 is less than the 160 * time_bins=16"]
    for at, text in enumerate(words):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)
    for kw, text in ((dict(clip_samples=L + 1), "clip_samples is misaligned"), (dict(time_bins=-4), "time_bins=-4"),
                     (dict(time_bins=17), "n_out=2600 is less than"), (dict(samples_out=S + 1, bins_out=0, time_bins=0),
                                                                       "clip_samples_out is misaligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    text = _header("lsm_hip_ragged_speed.h")                         # the order is stated in the header
    stated = [text.index(w) for w in ("what lsm_speed_f32 refuses", "a NULL clip_samples", "then a clip_samples that is not 4-byte",
                                      "a clip_samples_out, then a", "time_bins < 3", "then n_out < 160 * time_bins")]
    assert stated == sorted(stated)


# ---- the restatement of SPEC.md 1.18 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", DESIGNS)
def test_the_restatement_is_resample_poly_of_the_clip_alone_then_zeros(factor):
    from scipy.signal import resample_poly
    from lsm_speech_classifier_amd import frontend
    table = frontend.speed_design(factor)
    n_in, n_out = 2500, 2600
    lengths = [-3, 0, 1, 159, 160, 161, 1300, 1301, 1843, 1844, 2500, 2505]
    rng = np.random.default_rng(sum(factor.encode()))
    x = (rng.standard_normal((len(lengths), n_in)) * 0.1).astype(np.float32)
    dirty = x.copy()
    for b, n_b in enumerate(SRR.clamp_samples(lengths, n_in)):
        dirty[b, n_b:] = np.nan                                     # what lies behind a clip is never looked at
    out, samples, bins = SRR.perturb_ragged(dirty, lengths, [table], None, n_out, 16)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert out.tobytes() == SRR.perturb_ragged(x, lengths, [table], None, n_out, 16)[0].tobytes()
    for b, n_b in enumerate(SRR.clamp_samples(lengths, n_in)):
        whole = -(-int(n_b) * table.up // table.down)
        assert samples[b] == min(whole, n_out) and bins[b] == min(-(-int(samples[b]) // 160), 16)
        assert not out[b, samples[b]:].view(np.uint32).any()        # the bits of +0.0: no ring-out tail
        if n_b == 0:
            continue
        ref = resample_poly(x[b, :n_b].astype(np.float64), table.up, table.down)
        assert len(ref) == whole
        err, bound = np.abs(out[b, :samples[b]].astype(np.float64) - ref[:samples[b]]).max(), 2.0 ** -23 * np.abs(ref).max()
        print(f"{factor}: n_b={n_b}: n'={samples[b]}: max |y - ref| = {err:.3e} = {err / bound:.2f} of the bound")
        assert err <= bound
        # and 1.12's restatement of the clip alone, byte for byte
        assert out[b, :samples[b]].tobytes() == SR.perturb(x[b, :n_b], table, int(samples[b])).tobytes()
    cut = {"9/10": [10, 11], "1/2": [7, 8, 9, 10, 11]}.get(factor, [])
    assert [b for b in range(len(lengths)) if samples[b] == n_out and -(-min(max(lengths[b], 0), n_in) * table.up // table.down)
            > n_out] == cut


def test_the_restatement_copies_a_clip_without_a_design_and_clamps_rows():
    from lsm_speech_classifier_amd import frontend
    tables = [frontend.speed_design("9/10"), frontend.speed_design("11/10")]
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((4, 300)) * 0.1).astype(np.float32)
    x[2, 3], x[2, 4] = np.float32(-0.0), np.float32(np.nan)
    out, samples, bins = SRR.perturb_ragged(x, [200, 200, 250, 300], tables, [0, 7, -1, -5], 280, 1)
    assert samples.tolist() == [223, 182, 250, 280] and bins.tolist() == [1, 1, 1, 1]
    assert out[0, :223].tobytes() == SR.perturb(x[0, :200], tables[0], 223).tobytes()
    assert out[1, :182].tobytes() == SR.perturb(x[1, :200], tables[1], 182).tobytes()          # clamped to the last row
    assert out[2, :250].tobytes() == x[2, :250].tobytes() and not out[2, 250:].view(np.uint32).any()
    assert out[3].tobytes() == x[3, :280].tobytes()
    xi = np.array([[-32768, 1, 32767, 5]], dtype=np.int16)
    assert SRR.perturb_ragged(xi, [3], tables, [-1], 5, 3)[0].tolist() == [[-1.0, 2.0 ** -15, 32767 / 32768, 0.0, 0.0]]


# ---- AugmentChain.speed_ragged ------------------------------------------------------------------------------------------
class Stage:
    """A device stage that records its call (tests/test_augment_host.py): it hands back (its name, its input)."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def _call(self, *args, **kw):
        self.log.append((self.name, args, kw))
        return (self.name, args[0])

    perturb = reverb = mix = mix_ragged = _call

    def perturb_ragged(self, *args, **kw):
        self.log.append((self.name + "_ragged", args, kw))
        return (self.name, args[0]), "samples", "bins"


def test_speed_ragged_runs_ahead_of_apply_ragged_with_the_plans_arrays():
    from lsm_speech_classifier_amd import augment, frontend
    n = 12
    plans = augment.StepPlans(speed=frontend.speed_plan(n, 3, prob=0.5, seed=4), reverb=frontend.reverb_plan(n, 4, prob=0.5, seed=4),
                              mix=frontend.mix_plan(n, 3, 500, (0.0, 20.0), max_shift=40, level_db=(-6.0, 0.0), seed=4))
    log, x, lengths = [], object(), object()
    chain = augment.AugmentChain(speed=Stage(log, "speed"), reverb=Stage(log, "reverb"), mixer=Stage(log, "mix"))
    assert list(inspect.signature(chain.speed_ragged).parameters) == ["x", "lengths", "plans", "time_bins", "out"]
    y, samples, bins = chain.speed_ragged(x, lengths, plans, time_bins=40)
    assert (y, samples, bins) == (("speed", x), "samples", "bins")
    got = chain.apply_ragged(y, samples, plans._replace(speed=None))
    assert [name for name, _, _ in log] == ["speed_ragged", "reverb", "mix"]
    (_, a0, k0), (_, a1, _), (_, a2, _) = log
    assert len(a0) == 3 and a0[0] is x and a0[1] is lengths and a0[2] is plans.speed.choice and k0 == {"time_bins": 40, "out": None}
    assert a1[0] == ("speed", x) and a1[1] is plans.reverb.rows                     # each stage reads the one before
    m = plans.mix
    assert a2[0] == ("reverb", ("speed", x)) and a2[1] == "samples"                 # the mixer takes the new lengths
    assert all(g is w for g, w in zip(a2[2:], (m.snr_db, m.rows, m.offsets, m.shift, m.scale)))
    assert got == ("mix", ("reverb", ("speed", x)))
    # a caller's buffer goes through; without a speed plan nothing is launched; without the stage the plan is refused
    log.clear()
    chain.speed_ragged(x, lengths, plans, out="rows")
    assert log[0][2] == {"time_bins": None, "out": "rows"}
    log.clear()
    assert chain.speed_ragged(x, lengths, plans._replace(speed=None)) == (x, None, None) and not log
    with pytest.raises(ValueError, match="speed perturber"):
        augment.AugmentChain(reverb=Stage(log, "reverb")).speed_ragged(x, lengths, plans._replace(mix=None))
    # apply_ragged keeps its contract: a speed plan is still refused there, word for word
    with pytest.raises(ValueError) as e:
        chain.apply_ragged(x, lengths, plans)
    assert str(e.value) == "speed perturbation is not offered on ragged batches: a speed factor changes a clip's bin count"
    assert not log


def test_the_builder_and_the_pipeline_take_the_speed_stage():
    import create_dataset as cd
    from lsm_speech_classifier_amd import pipeline
    assert inspect.signature(cd.create_variable_length_dataset).parameters["speed"].default is None
    sig = inspect.signature(pipeline.features_from_utterances).parameters
    assert sig["speed"].default is None and list(sig)[-1] == "speed"             # behind the parameters it had


# ---- the scripts' flags -------------------------------------------------------------------------------------------------
def _parser(cd):
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--resample", default="host")
    for add in (cd.add_augment_flags, cd.add_reverb_flags, cd.add_speed_flags, cd.add_mask_flags, cd.add_variable_length_flags):
        add(ap)
    return ap


SPEED = ["--speed-factors", "0.9,1.0,1.1", "--speed-prob", "0.5", "--augment-seed", "9"]
CHAIN_FLAGS = {"the corruption flags": ["--noise-dir", "synthetic", "--snr-db", "5,15"], "--rir-dir": ["--rir-dir", "synthetic"],
               "the mask flags": ["--time-masks", "1", "--time-mask-width", "5"]}


def test_the_new_flag_lets_the_speed_flags_through_and_every_refusal_of_today_still_fires(monkeypatch):
    import create_dataset as cd
    ap = _parser(cd)
    assert ap.parse_args([]).speed_variable_length is False
    both = ["--variable-length", "--augment-variable-length", "--speed-variable-length"]
    a = ap.parse_args(both + SPEED)
    assert a.speed_variable_length is True
    cd.check_variable_length_args(a)
    assert cd.speed_from_args(a) == dict(factors=["0.9", "1.0", "1.1"], prob=0.5, seed=9)
    every = sum(CHAIN_FLAGS.values(), [])
    a = ap.parse_args(both + SPEED + every + ["--trim-silence", "30"])
    cd.check_variable_length_args(a)
    assert cd.speed_from_args(a)["factors"] == ["0.9", "1.0", "1.1"] and cd.trim_from_args(a)["top_db"] == 30.0
    cd.check_variable_length_args(ap.parse_args(both))              # the flag alone changes nothing
    # without the new flag: today's refusals, word for word
    for flags in (["--variable-length"], ["--variable-length", "--augment-variable-length"],
                  ["--variable-length", "--speed-variable-length"]):
        with pytest.raises(SystemExit) as e:
            cd.check_variable_length_args(ap.parse_args(flags + SPEED))
        assert str(e.value) == "--variable-length does not combine with --speed-factors"
    with pytest.raises(SystemExit) as e:
        cd.check_variable_length_args(ap.parse_args(["--variable-length", "--augment-variable-length"] + SPEED + every))
    assert str(e.value) == "--variable-length does not combine with --speed-factors"
    for name, flags in CHAIN_FLAGS.items():
        with pytest.raises(SystemExit) as e:
            cd.check_variable_length_args(ap.parse_args(["--variable-length"] + flags))
        assert str(e.value) == f"--variable-length does not combine with {name}"
        with pytest.raises(SystemExit) as e:                        # the speed flag does not stand in for the chain's
            cd.check_variable_length_args(ap.parse_args(["--variable-length", "--speed-variable-length"] + flags))
        assert str(e.value) == f"--variable-length does not combine with {name}"
    with pytest.raises(SystemExit) as e:
        cd.check_variable_length_args(ap.parse_args(["--variable-length"] + every + SPEED))
    assert str(e.value) == "--variable-length does not combine with the corruption flags, --rir-dir, --speed-factors, the mask flags"
    # what stays refused with both flags
    for flags, text in ((["--packed"], "--packed"), (["--resample", "device"], "--resample device")):
        with pytest.raises(SystemExit, match="--variable-length does not combine with " + text):
            cd.check_variable_length_args(ap.parse_args(both + SPEED + flags))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--variable-length runs in one process"):
        cd.check_variable_length_args(ap.parse_args(both + SPEED))
    monkeypatch.delenv("WORLD_SIZE")
    for bad in (["--speed-factors", "0.9", "--speed-prob", "2"], ["--speed-factors", "1.0"]):     # the flags' own checks
        with pytest.raises(SystemExit):
            cd.speed_from_args(ap.parse_args(both + bad))


def test_main_forwards_the_new_flag_only_when_it_is_set(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, *k, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, augment_variable_length=True,
                          speed_variable_length=True, speed_factors="0.9,1.1", trim_silence=30.0)
    assert calls[0][6:] == ["--speed-factors", "0.9,1.1", "--speed-prob", "1.0", "--augment-seed", "42", "--variable-length",
                            "--max-seconds", "1.0", "--augment-variable-length", "--speed-variable-length", "--trim-silence", "30.0",
                            "--trim-pad-ms", "30.0", "--trim-min-ms", "30.0"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, variable_length=True, augment_variable_length=True, trim_silence=30.0)
    assert calls[0][6:] == ["--variable-length", "--max-seconds", "1.0", "--augment-variable-length", "--trim-silence", "30.0",
                            "--trim-pad-ms", "30.0", "--trim-min-ms", "30.0"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, speed_variable_length=True)      # nothing without --variable-length
    assert calls[0][1:] == [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, speed_factors="0.9,1.1")
    assert "speed_variable_length" not in calls[0][2]               # the in-memory route's program is what it was
