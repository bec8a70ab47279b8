"""The masked and the ragged one-launch step inside the pipeline: `HotPath(fused_forms=True)` with 4 hardware queues routes
masked steps, and steps with a mixer in front of them, to `step_fused(mask=...)`, and `features_from_utterances(fused=True)`
routes its batches to `step_fused_ragged`; the rows are byte for byte those of the default routes.  Both switches are off by
default (profiles/step_fused_forms.txt), and without them nothing is routed differently."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_fused_forms_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu
_built = {}


def _case(oracle_c):
    if not _built:
        from lsm_speech_classifier_amd import frontend, snn, synth
        fe = frontend.SpikeFrontEnd(128, "gammatone", thresholds=REF.thresholds(4), time_bins=16, n_samples=2560)
        net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, 128, 16, 4, 160, 384))
        audio = np.ascontiguousarray(synth.class_chirps(np.arange(48) % 12, seed=5, n_samples=2560))
        masks = frontend.mask_plan(48, 128, 16, freq_masks=2, freq_width=12, time_masks=1, time_width=4, prob=0.8, seed=7)
        _built["case"] = fe, net, audio, masks
    return _built["case"]


def _run(monkeypatch, queues, fused_forms, fe, net, audio, masks, mixer=None, mixes=None):
    """`HotPath.run` over 6 steps of 8 clips with `queues` hardware queues; returns (rows, calls of step_fused with a mask,
    calls without)."""
    from lsm_speech_classifier_amd import pipeline
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", str(queues))
    monkeypatch.setattr(pipeline, "configure_hardware_queues", lambda n=12: queues)
    calls = []
    real = pipeline.step_fused
    monkeypatch.setattr(pipeline, "step_fused", lambda *a, **k: (calls.append(k.get("mask") is not None), real(*a, **k))[1])
    hp = pipeline.HotPath(fe, net, streams=6, mixer=mixer, fused_forms=fused_forms)
    assert hp.hw_queues == queues
    parts = range(0, 48, 8)
    rows = hp.run([audio[lo:lo + 8] for lo in parts], masks=[masks.part(lo, lo + 8) for lo in parts],
                  mixes=None if mixes is None else [mixes.part(lo, lo + 8) for lo in parts])
    monkeypatch.setattr(pipeline, "step_fused", real)
    return rows.cpu().numpy(), sum(calls), len(calls) - sum(calls)


def test_masked_steps_take_the_fused_launch_with_four_queues(oracle_c, monkeypatch):
    fe, net, audio, masks = _case(oracle_c)
    want, masked, plain = _run(monkeypatch, 12, False, fe, net, audio, masks)
    assert (masked, plain) == (0, 0) and want.any()
    got, masked, plain = _run(monkeypatch, 4, True, fe, net, audio, masks)
    assert (masked, plain) == (6, 0)
    assert got.tobytes() == want.tobytes()
    off, masked, plain = _run(monkeypatch, 4, False, fe, net, audio, masks)         # the default: the two launches
    assert (masked, plain) == (0, 0) and off.tobytes() == want.tobytes()
    import torch
    from lsm_speech_classifier_amd import pipeline
    unmasked = pipeline.step_fused(fe, net, torch.from_numpy(audio[:8]).cuda()).cpu().numpy()
    assert not np.array_equal(unmasked, want[:8])


def test_mixed_and_masked_steps_take_the_fused_launch_with_four_queues(oracle_c, monkeypatch):
    from lsm_speech_classifier_amd import frontend
    fe, net, audio, masks = _case(oracle_c)
    noise = (np.random.default_rng(62).standard_normal((3, 4097)) * 0.05).astype(np.float32)
    mixer = frontend.NoiseMixer(noise)
    mixes = frontend.mix_plan(48, 3, 4097, (0.0, 20.0), max_shift=400, level_db=(-6.0, 0.0), seed=9)
    want, masked, plain = _run(monkeypatch, 12, False, fe, net, audio, masks, mixer, mixes)
    assert (masked, plain) == (0, 0)
    clean = _run(monkeypatch, 12, False, fe, net, audio, masks)[0]
    assert not np.array_equal(want, clean)                                           # the mixer changed the rows
    got, masked, plain = _run(monkeypatch, 4, True, fe, net, audio, masks, mixer, mixes)
    assert (masked, plain) == (6, 0) and got.tobytes() == want.tobytes()
    off, masked, plain = _run(monkeypatch, 4, False, fe, net, audio, masks, mixer, mixes)
    assert (masked, plain) == (0, 0) and off.tobytes() == want.tobytes()


def test_utterances_take_the_ragged_fused_launch(oracle_c, monkeypatch):
    """12 utterances of 3 to 16 bins (481 to 2560 samples), batches of 8: two ragged fused launches, the rows of the two
    launches per batch."""
    from lsm_speech_classifier_amd import pipeline
    fe, net, audio, _ = _case(oracle_c)
    lengths = [2560, 481, 1000, 2401, 640, 1599, 2000, 800, 1280, 2559, 500, 1920]
    utts = [audio[i, :n].copy() for i, n in enumerate(lengths)]
    want = pipeline.features_from_utterances(utts, fe, net, None, batch=8).cpu().numpy()
    calls = []
    real = pipeline.step_fused_ragged
    monkeypatch.setattr(pipeline, "step_fused_ragged", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    again = pipeline.features_from_utterances(utts, fe, net, None, batch=8).cpu().numpy()
    assert not calls and again.tobytes() == want.tobytes()
    got = pipeline.features_from_utterances(utts, fe, net, None, batch=8, fused=True).cpu().numpy()
    assert len(calls) == 2 and got.tobytes() == want.tobytes()
    assert want.any() and len({want[i].tobytes() for i in range(12)}) == 12
