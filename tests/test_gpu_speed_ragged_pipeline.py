"""Speed perturbation on clips of different lengths, end to end (SPEC.md 1.18): `pipeline.features_from_utterances(speed=...)`
and `create_dataset.py --variable-length --augment-variable-length --speed-variable-length`.

Row r must be, bit for bit, the chain on utterance r ALONE: `SpeedPerturber.perturb` on the utterance at its own length and
n_out = n', cut at the row, and that one clip through `features_from_utterances` with its own slice of every other plan --
launches in which no other clip, no padding and no row stride takes part.  A front end of 40 bins (6400 samples), 128
gammatone filters and the small reservoir of the one-launch step's tests, so that `fused=True` takes the ragged one-launch
step; seven utterances of 3 to 40 bins, among them an unperturbed one, one that 9/10 brings exactly to the row's 40 bins and
one that it pushes past them."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_fused_forms_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, TB, F = 160, 40, 128
BINS = [3, 4, 5, 20, 33, 36, 40]
FACTORS = ["9/10", 1, "11/10"]
CHOICE = [2, 0, -1, 1, 2, 0, 0]               # 11/10, 9/10, left alone, factor 1, 11/10, 9/10 to exactly 40 bins, 9/10 and cut
NEW_BINS = [3, 5, 5, 20, 30, 40, 40]
MASK = dict(freq_masks=1, freq_width=12, time_masks=1, time_width=2, prob=0.9, seed=11)     # a clip of 3 bins keeps a bin
_built = {}


def _setup(oracle_c):
    if not _built:
        from lsm_speech_classifier_amd import frontend, snn, synth
        fe = frontend.SpikeFrontEnd(F, "gammatone", thresholds=REF.thresholds(4), time_bins=TB, n_samples=HOP * TB)
        net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, F, TB, 4, HOP, 64))
        clips = synth.class_chirps(np.arange(len(BINS)), seed=1234, noise=0.001)
        # the short ones from inside the chirp, the long ones from its onset, so that the trimmer cuts those
        utts = [np.ascontiguousarray(c[(1600 if b >= 20 else 6400):][:HOP * b]) for c, b in zip(clips, BINS)]
        rir, rir_lengths = synth.room_responses(3, seed=5)
        noise = synth.white_noise(2, seed=3, n_samples=5000) * np.float32(0.1)
        _built["all"] = (fe, net, utts, frontend.SpeedPerturber(FACTORS), frontend.SpeedPlan(np.asarray(CHOICE, dtype=np.int32)),
                         frontend.Reverberator(rir, rir_lengths), frontend.NoiseMixer(noise), frontend.SilenceTrimmer(30.0, 1, 4))
    return _built["all"]


def _played_alone(sp, u, choice):
    """Utterance ``u`` played at its speed in a launch of its own shape (`lsm_speed_f32`: n_in = len(u), n_out = n' =
    ceil(len(u) * up / down)), cut at the row's 6400 samples."""
    row = int(sp.row_of_choice[choice]) if choice >= 0 else -1
    up, down = (1, 1) if row < 0 else (int(v) for v in sp.designs[row, :2])
    whole = -(-len(u) * up // down)
    return sp.perturb(u[None].copy(), [choice], n_out=whole).cpu().numpy()[0, :HOP * TB]


def test_the_host_lengths_are_the_formula_and_the_plan_covers_the_cases(oracle_c):
    from lsm_speech_classifier_amd import frontend
    fe, net, utts, sp, paces, *_ = _setup(oracle_c)
    new = frontend.speed_ragged_lengths(np.asarray(BINS) * HOP, paces.choice, sp, HOP * TB)
    assert new.tolist() == [437, 712, 800, 3200, 4800, 6400, 6400] and (-(-new // HOP)).tolist() == NEW_BINS
    assert -(-BINS[5] * HOP * 10 // 9) == HOP * TB and -(-BINS[6] * HOP * 10 // 9) > HOP * TB
    assert [len(_played_alone(sp, u, c)) for u, c in zip(utts, CHOICE)] == new.tolist()


@pytest.mark.parametrize("chain", ["speed", "speed-trim-reverb-mix-mask"])
def test_the_rows_equal_the_chain_on_each_utterance_alone(oracle_c, monkeypatch, chain):
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net, utts, sp, paces, rv, mixer, trimmer = _setup(oracle_c)
    n = len(utts)
    whole = chain != "speed"
    reverbs = frontend.reverb_plan(n, rv.n_rows, prob=0.7, seed=4)
    mixes = frontend.mix_plan(n, mixer.n_rows, mixer.noise_len, (5.0, 15.0), max_shift=400, level_db=(-6.0, 0.0), seed=4)
    planned = []

    def plan_masks(bins):                                           # called once per run, with the final host bins
        planned.append((np.array(bins), frontend.mask_plan_ragged(bins, F, TB, **MASK)))
        return planned[-1][1]

    kw = dict(trim=trimmer, reverb=(rv, reverbs), corrupt=(mixer, mixes), mask=plan_masks) if whole else {}
    form = "ragged-masked" if whole else "ragged"
    assert pipeline.step_fused_supported(fe, net, 3, form)
    calls = []
    real = pipeline.step_fused_ragged
    monkeypatch.setattr(pipeline, "step_fused_ragged", lambda *a, **k: (calls.append(len(a[2])), real(*a, **k))[1])
    got = {fused: pipeline.features_from_utterances(utts, fe, net, None, batch=3, fused=fused, speed=(sp, paces), **kw).cpu().numpy()
           for fused in (False, True)}
    assert calls == [3, 3, 1], "fused=True did not take the ragged one-launch step"
    if whole:
        assert len(planned) == 2 and planned[0][1].time.tobytes() == planned[1][1].time.tobytes()
        final = planned[0][0]
        assert (final <= NEW_BINS).all() and (final >= 3).all() and (final < NEW_BINS).sum() >= 3, "hardly an utterance trims"
    # every utterance alone: played in a launch of its own, then the same route with its own slice of every plan
    want = []
    for r, u in enumerate(utts):
        alone = dict(kw)
        if whole:
            alone.update(reverb=(rv, reverbs.part(r, r + 1)), corrupt=(mixer, mixes.part(r, r + 1)), mask=planned[0][1].part(r, r + 1))
        want.append(pipeline.features_from_utterances([_played_alone(sp, u, CHOICE[r])], fe, net, None, **alone).cpu().numpy()[0])
    want = np.stack(want)
    for fused in (False, True):
        for r in range(n):
            assert got[fused][r].view(np.uint32).tobytes() == want[r].view(np.uint32).tobytes(), f"fused={fused}, utterance {r}"
    live = want[want.any(axis=1)]                                   # the reference tells the clips apart
    assert len(live) >= (4 if whole else n) and len({w.tobytes() for w in live}) == len(live)
    # the speed stage matters, and without it not one row changes
    plain = pipeline.features_from_utterances(utts, fe, net, None, batch=3, **({} if not whole else dict(kw, mask=None)))
    none = pipeline.features_from_utterances(utts, fe, net, None, batch=3, speed=None, **({} if not whole else dict(kw, mask=None)))
    assert plain.cpu().numpy().tobytes() == none.cpu().numpy().tobytes()
    if not whole:
        moved = [r for r in range(n) if got[False][r].tobytes() != plain.cpu().numpy()[r].tobytes()]
        assert moved == [r for r, c in enumerate(CHOICE) if c in (0, 2)]             # factor 1 and no factor: the same rows


def test_the_speed_stage_refuses_a_short_clip_and_a_short_plan_before_any_launch(oracle_c):
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net, utts, sp, paces, *_ = _setup(oracle_c)
    fast = frontend.SpeedPerturber(["2", "9/10"])
    with pytest.raises(ValueError, match="utterance 1 has 4 time bins and 2 at its speed"):
        pipeline.features_from_utterances(utts[:3], fe, net, None, speed=(fast, frontend.SpeedPlan(np.array([1, 0, -1], np.int32))))
    with pytest.raises(ValueError, match="the speed plan covers 2 clips, audio has 3"):
        pipeline.features_from_utterances(utts[:3], fe, net, None, speed=(sp, paces.part(0, 2)))
    with pytest.raises(ValueError, match="speed perturber"):
        pipeline.features_from_utterances(utts[:3], fe, net, None, speed=(None, paces.part(0, 3)))


def test_create_dataset_perturbs_variable_length_clips(oracle_c, tmp_path):
    """`create_dataset.py --variable-length --augment-variable-length --speed-variable-length --speed-factors 0.9,1.0,1.1
    --synthetic-per-class 2`: File 1's n_steps are the host formula times n_thr, its rows those of the same stage through the
    Python API."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend
    flags = ["--variable-length", "--augment-variable-length", "--speed-variable-length", "--speed-factors", "0.9,1.0,1.1",
             "--synthetic-per-class", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--n-filters", "16"] + flags, capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(str(tmp_path / cd.OUTPUT_FILE)) as data:
        X, n_steps, y = data["X_spikes"], data["n_steps"], data["y_labels"]
    clips, labels = cd._synthetic_utterances(list(cd.COMMANDS), 2, 100)
    audio, bins = frontend.pack_utterances(clips, 100)
    factors, paces = cd.speeds(dict(factors=["0.9", "1.0", "1.1"], prob=1.0, seed=42), len(clips))
    sp = frontend.SpeedPerturber(factors)
    new = frontend.speed_ragged_lengths(bins.astype(np.int64) * HOP, paces.choice, sp, 16000)
    new_bins = -(-new // HOP)
    n_thr = len(cd.SPIKE_THRESHOLDS)
    assert n_steps.tolist() == (new_bins * n_thr).tolist() and y.tolist() == list(labels)
    assert set(paces.choice.tolist()) == {0, 1, 2} and (new_bins != bins).sum() >= 10 and new_bins.max() == 100
    fe = frontend.SpikeFrontEnd(16, "gammatone", redundancy=cd.REDUNDANCY_FACTOR, thresholds=cd.SPIKE_THRESHOLDS,
                                gap=cd.HYSTERESIS_GAP, time_bins=100, n_samples=16000)
    x, samples, dev_bins = sp.perturb_ragged(audio, bins.astype(np.int64) * HOP, paces.choice, time_bins=100)
    assert samples.cpu().tolist() == new.tolist() and dev_bins.cpu().tolist() == new_bins.tolist()
    want = fe.encode_ragged(x, new_bins.astype(np.int32))[0].cpu().numpy()
    assert X.shape == want.shape and np.array_equal(X, want) and X.any()
    assert not np.array_equal(X, fe.encode_ragged(audio, bins)[0].cpu().numpy())
    # without the new flag the route refuses the speed flags as before, before any device work
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--n-filters", "16"]
                       + [f for f in flags if f != "--speed-variable-length"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "--variable-length does not combine with --speed-factors" in r.stderr
