"""The augmentation chain on clips of different lengths, end to end (SPEC.md 1.16): `pipeline.features_from_utterances(trim=...,
reverb=..., corrupt=..., mask=...)` and `create_dataset.py --variable-length --augment-variable-length`.

Row r must be, bit for bit, the clip-alone chain on utterance r: trim it, `lsm_reverb_f32` and `lsm_mix_f32` at its own
(trimmed) length, the masked front end built for that length, the reservoir run of that length -- launches in which no other
clip, no padding and no row stride takes part.  A dozen synthetic utterances of 0.3 to 1.0 s, 128 gammatone filters and the
small reservoir of the one-launch step's tests, so that `fused=True` takes `lsm_step_fused_ragged_masked_f64`."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402
import step_fused_forms_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, TB, F = 160, 100, 128
MASK = dict(freq_masks=1, freq_width=12, time_masks=2, time_width=8, prob=0.9, seed=11)
_built = {}


def _utterances():
    """Twelve quiet-background chirps (so that the trimmer finds their speech) cut to seeded lengths of 0.3 to 1.0 s."""
    from lsm_speech_classifier_amd import synth
    clips = synth.class_chirps(np.arange(12), seed=1234, noise=0.001)
    lengths = np.random.RandomState(8).randint(4800, 16001, size=12)
    lengths[0], lengths[1] = 16000, 4800
    return [np.ascontiguousarray(c[:n]) for c, n in zip(clips, lengths)]


def _setup(oracle_c):
    if not _built:
        from lsm_speech_classifier_amd import frontend, snn, synth
        fe = frontend.SpikeFrontEnd(F, "gammatone", thresholds=REF.thresholds(4), time_bins=TB, n_samples=HOP * TB)
        net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, F, TB, 4, HOP, 64))
        rir, rir_lengths = synth.room_responses(3, seed=5)
        noise = synth.white_noise(2, seed=3, n_samples=5000) * np.float32(0.1)
        _built["all"] = (fe, net, _utterances(), frontend.Reverberator(rir, rir_lengths), frontend.NoiseMixer(noise),
                         frontend.SilenceTrimmer(30.0, 1, 4))
    return _built["all"]


def _front_end(T):
    from lsm_speech_classifier_amd import frontend
    if ("fe", T) not in _built:
        _built["fe", T] = frontend.SpikeFrontEnd(F, "gammatone", thresholds=REF.thresholds(4), time_bins=T, n_samples=HOP * T)
    return _built["fe", T]


def _alone(torch, fe, net, u, trimmer, rv, mixer, reverbs, mixes, mask, r):
    """Utterance r through the chain ALONE -> (its feature row, its bins): every launch at the clip's own length."""
    from lsm_speech_classifier_amd import frontend
    row = np.zeros((1, HOP * TB), np.float32)
    row[0, :len(u)] = u
    T = -(-len(u) // HOP)
    x = torch.from_numpy(row).cuda()
    if trimmer is not None:
        x, kept, _ = trimmer.trim(x, [T * HOP], time_bins=TB)
        T = int(kept.cpu()[0])
    x = x[:, :HOP * T].contiguous()
    if reverbs is not None:
        x = rv.reverb(x, reverbs.rows[r:r + 1])                     # lsm_reverb_f32, n_in = n_out = 160 T
    if mixes is not None:
        x = mixer.mix(x, mixes.snr_db[r:r + 1], mixes.rows[r:r + 1], mixes.offsets[r:r + 1], mixes.shift[r:r + 1],
                      mixes.scale[r:r + 1])                         # lsm_mix_f32 at 160 T samples
    plan = None
    if mask is not None:
        plan = frontend.MaskPlan(mask.freq[r:r + 1], MR.words_of(MR.bits_of(mask.time[r:r + 1], T)))
    raster = _front_end(T).encode(x, mask=plan)
    feats = net.run_batch(raster, None)[0]
    torch.cuda.synchronize()
    return feats[0].cpu().numpy(), T


def test_the_whole_chain_equals_the_clip_alone_chain(oracle_c, monkeypatch):
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net, utts, rv, mixer, trimmer = _setup(oracle_c)
    n = len(utts)
    reverbs = frontend.reverb_plan(n, rv.n_rows, prob=0.7, seed=4)
    mixes = frontend.mix_plan(n, mixer.n_rows, mixer.noise_len, (5.0, 15.0), max_shift=1600, level_db=(-6.0, 0.0), seed=4)
    planned = []

    def plan_masks(bins):                                           # called once, behind the one read-back of the trimmed bins
        planned.append(frontend.mask_plan_ragged(bins, F, TB, **MASK))
        return planned[-1]

    assert pipeline.step_fused_supported(fe, net, 5, "ragged-masked")
    calls = []
    real = pipeline.step_fused_ragged
    monkeypatch.setattr(pipeline, "step_fused_ragged", lambda *a, **k: (calls.append(k.get("mask")), real(*a, **k))[1])
    got = {}
    for fused in (False, True):
        got[fused] = pipeline.features_from_utterances(utts, fe, net, None, batch=5, fused=fused, trim=trimmer, reverb=(rv, reverbs),
                                                       corrupt=(mixer, mixes), mask=plan_masks).cpu().numpy()
    assert len(planned) == 2 and planned[0].time.tobytes() == planned[1].time.tobytes()
    assert len(calls) == 3 and all(m is not None for m in calls), "fused=True did not take the masked ragged step"
    want, bins = zip(*[_alone(torch, fe, net, u, trimmer, rv, mixer, reverbs, mixes, planned[0], r) for r, u in enumerate(utts)])
    want, bins = np.stack(want), np.array(bins)
    whole = np.array([-(-len(u) // HOP) for u in utts])
    assert (bins >= 4).all() and (bins < whole).sum() >= 6, "hardly an utterance trims"
    assert MR.bits_of(planned[0].time, TB).any(axis=1).sum() >= 6 and (reverbs.rows >= 0).sum() >= 4
    for b, T in enumerate(bins):
        assert not MR.bits_of(planned[0].time[b], 128)[T:].any(), "the masks were not planned for the trimmed bins"
    for fused in (False, True):
        assert got[fused].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), f"fused={fused}"
    live = want[want.any(axis=1)]
    assert len(live) >= 6 and len({w.tobytes() for w in live}) == len(live)      # the reference tells the clips apart
    # each stage matters: without it the rows differ; a MaskPlan given as such is taken as the callable's
    for drop in ("trim", "reverb", "corrupt", "mask"):
        kw = dict(trim=trimmer, reverb=(rv, reverbs), corrupt=(mixer, mixes), mask=planned[0])
        kw[drop] = None
        other = pipeline.features_from_utterances(utts, fe, net, None, **kw).cpu().numpy()
        assert not np.array_equal(other, want), drop
    same = pipeline.features_from_utterances(utts, fe, net, None, trim=trimmer, reverb=(rv, reverbs), corrupt=(mixer, mixes),
                                             mask=planned[0]).cpu().numpy()
    assert same.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="mask plan covers"):
        pipeline.features_from_utterances(utts, fe, net, None, mask=frontend.mask_plan_ragged(whole[:5], F, TB, **MASK))


def test_reverberation_on_padded_rows_is_the_clip_alone_up_to_its_end(oracle_c):
    """`lsm_reverb_f32` with n_out = n_in is causal: the first L_b output samples of a padded row are those of the clip alone,
    bit for bit, whatever lies behind the clip (here: another signal)."""
    import torch
    fe, net, utts, rv, mixer, trimmer = _setup(oracle_c)
    rows = np.array([0, 1, 2, -1, 2, 0, 1, 0, -1, 2, 1, 0], dtype=np.int32)
    rng = np.random.default_rng(1)
    padded = (rng.standard_normal((12, HOP * TB)) * 0.3).astype(np.float32)          # what lies behind a clip is not silence
    for r, u in enumerate(utts):
        padded[r, :len(u)] = u
    got = rv.reverb(torch.from_numpy(padded).cuda(), rows)
    quiet = padded.copy()
    for r, u in enumerate(utts):
        quiet[r, len(u):] = 0.0
    got_quiet = rv.reverb(torch.from_numpy(quiet).cuda(), rows)
    torch.cuda.synchronize()
    got, got_quiet = got.cpu().numpy(), got_quiet.cpu().numpy()
    tails = 0
    for r, u in enumerate(utts):
        alone = rv.reverb(torch.from_numpy(u[None].copy()).cuda(), rows[r:r + 1]).cpu().numpy()[0]
        assert got[r, :len(u)].tobytes() == alone.tobytes() == got_quiet[r, :len(u)].tobytes(), f"utterance {r}"
        tails += bool(len(u) < HOP * TB and got_quiet[r, len(u):].any())
    assert tails >= 6, "no row has a reverberation tail behind its clip"


def test_without_the_chain_the_rows_are_the_ragged_front_end_and_run(oracle_c):
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline
    fe, net, utts, *_ = _setup(oracle_c)
    plain = pipeline.features_from_utterances(utts, fe, net, None)
    none = pipeline.features_from_utterances(utts, fe, net, None, trim=None, corrupt=None, reverb=None, mask=None)
    audio, bins = frontend.pack_utterances(utts, TB)
    raster, steps = fe.encode_ragged(audio, bins)
    want = net.run_batch(raster, None, lengths=steps)[0]
    torch.cuda.synchronize()
    assert torch.equal(plain, none) and torch.equal(plain, want) and bool(plain.any())


def test_create_dataset_augments_variable_length_clips(oracle_c, tmp_path):
    """`create_dataset.py --variable-length --augment-variable-length --synthetic-per-class 2 --snr-db 5,15 --noise-dir
    synthetic --time-masks 1 --time-mask-width 5`: File 1's rows are those of the same chain through the Python API."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend
    flags = ["--variable-length", "--augment-variable-length", "--synthetic-per-class", "2", "--snr-db", "5,15", "--noise-dir",
             "synthetic", "--time-masks", "1", "--time-mask-width", "5"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--n-filters", "16"] + flags, capture_output=True,
                       text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(str(tmp_path / cd.OUTPUT_FILE)) as data:
        X, n_steps, y = data["X_spikes"], data["n_steps"], data["y_labels"]
    clips, labels = cd._synthetic_utterances(list(cd.COMMANDS), 2, 100)
    fe = frontend.SpikeFrontEnd(16, "gammatone", redundancy=cd.REDUNDANCY_FACTOR, thresholds=cd.SPIKE_THRESHOLDS,
                                gap=cd.HYSTERESIS_GAP, time_bins=100, n_samples=16000)
    audio, bins = frontend.pack_utterances(clips, 100)
    augment = dict(noise_dir="synthetic", snr_db=(5.0, 15.0), time_shift_ms=0.0, level_db=0.0, seed=42)
    bank, mixes = cd.corruption(augment, len(clips))
    plan = frontend.mask_plan_ragged(bins, 16, 100, time_masks=1, time_width=5, seed=42)
    x = frontend.NoiseMixer(bank).mix_ragged(audio, bins.astype(np.int64) * HOP, mixes.snr_db, mixes.rows, mixes.offsets, mixes.shift,
                                             mixes.scale)
    want = fe.encode_ragged(x, bins, mask=plan)[0].cpu().numpy()
    assert n_steps.tolist() == (bins * 4).tolist() and y.tolist() == list(labels)
    assert X.shape == want.shape and np.array_equal(X, want) and X.any()
    clean = fe.encode_ragged(audio, bins)[0].cpu().numpy()
    assert not np.array_equal(X, clean)
    # without the new flag the route refuses the same flags as before, before any device work
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--n-filters", "16"]
                       + [f for f in flags if f != "--augment-variable-length"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "--variable-length does not combine with the corruption flags, the mask flags" in r.stderr
