"""One batch with all four plans at once -- speed, reverberation, mixer, mask -- through every topology of `HotPath`: serial,
rotation, two stages and the fused-forms route with 4 hardware queues.  The rows are byte for byte those of the stages called
directly in the recipe's order, a following step without plans gives the clean rows, and `run()` carries the four plan lists
batch by batch.  The shapes are those of tests/test_gpu_step_fused_pipeline.py, the smallest the fused step serves."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_fused_forms_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu
_built = {}
N, B = 20, 8                                    # three batches: 8, 8 and 4 clips
TOPOLOGIES = {"serial": (12, dict(streams=1)), "rotation": (12, dict(streams=3, fe_streams=0)), "two-stage": (12, {}),
              "fused": (4, dict(streams=6, fused_forms=True))}


def _case(oracle_c):
    """Front end, reservoir, stages, clips, their plans, and the rows (clean, augmented) computed directly, once."""
    if not _built:
        import torch
        from lsm_speech_classifier_amd import augment, frontend, snn, synth
        fe = frontend.SpikeFrontEnd(128, "gammatone", thresholds=REF.thresholds(4), time_bins=16, n_samples=2560)
        net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, 128, 16, 4, 160, 384))
        audio = np.ascontiguousarray(synth.class_chirps(np.arange(N) % 12, seed=5, n_samples=2560))
        rng = np.random.default_rng(63)
        rir = (rng.standard_normal((3, 200)) * 0.3 * np.exp(-np.arange(200) / 40.0)[None, :]).astype(np.float32)
        rir[:, 0] = 1.0
        sp = frontend.SpeedPerturber(["0.9", "1.0", "1.1"])
        rv = frontend.Reverberator(rir, np.array([200, 60, 9], dtype=np.int32))
        mixer = frontend.NoiseMixer((rng.standard_normal((3, 4097)) * 0.05).astype(np.float32))
        plans = augment.StepPlans(
            speed=frontend.SpeedPlan(np.resize(np.array([0, -1, 2, 1, 2], dtype=np.int32), N)),
            reverb=frontend.ReverbPlan(np.resize(np.array([1, 0, -1, 2], dtype=np.int32), N)),
            mix=frontend.mix_plan(N, 3, 4097, (0.0, 20.0), max_shift=400, level_db=(-6.0, 0.0), seed=9),
            mask=frontend.mask_plan(N, 128, 16, freq_masks=2, freq_width=12, time_masks=1, time_width=4, prob=0.8, seed=7))
        assert plans.mix.shift.any() and (plans.mix.scale != 1).any() and plans.mask.freq.any() and plans.mask.time.any()
        clean, want = [], []
        for lo in range(0, N, B):
            x, p = torch.from_numpy(audio[lo:lo + B]).cuda(), plans.part(lo, lo + B)
            m = p.mix
            y = mixer.mix(rv.reverb(sp.perturb(x, p.speed.choice), p.reverb.rows), m.snr_db, m.rows, m.offsets, m.shift, m.scale)
            want.append(net.run_batch(fe.encode(y, mask=p.mask))[0].cpu().numpy())
            clean.append(net.run_batch(fe.encode(x))[0].cpu().numpy())
        clean, want = np.concatenate(clean), np.concatenate(want)
        assert want.any() and clean.any() and not any(np.array_equal(want[lo:lo + B], clean[lo:lo + B]) for lo in range(0, N, B))
        _built["case"] = fe, net, dict(speed=sp, reverb=rv, mixer=mixer), audio, plans, clean, want
    return _built["case"]


@pytest.mark.parametrize("topology", list(TOPOLOGIES))
def test_a_step_with_all_four_plans_gives_the_rows_of_the_stages_called_directly(oracle_c, monkeypatch, topology):
    from lsm_speech_classifier_amd import pipeline
    fe, net, stages, audio, plans, clean, want = _case(oracle_c)
    queues, kw = TOPOLOGIES[topology]
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", str(queues))
    monkeypatch.setattr(pipeline, "configure_hardware_queues", lambda n=12: queues)
    fused = []
    real = pipeline.step_fused
    monkeypatch.setattr(pipeline, "step_fused", lambda *a, **k: (fused.append("mask" in k), real(*a, **k))[1])
    hp = pipeline.HotPath(fe, net, **stages, **kw)
    assert hp.hw_queues == queues and hp.fused_step == (topology == "fused")
    assert (hp.n_streams, hp.n_fe_streams) == {"serial": (1, 0), "rotation": (3, 0), "two-stage": (6, 5), "fused": (6, 5)}[topology]

    def rows_of(x, **step):
        feats, st = hp.submit(x, **step)
        st.synchronize()
        return feats.cpu().numpy().tobytes()

    first = plans.part(0, B)
    assert rows_of(audio[:B], speed=first.speed, reverb=first.reverb, mix=first.mix, mask=first.mask) == want[:B].tobytes()
    assert rows_of(audio[:B]) == clean[:B].tobytes()                    # a step without plans launches no stage
    assert rows_of(audio[:B], mix=first.mix, speed=first.speed, mask=first.mask, reverb=first.reverb) == want[:B].tobytes()
    assert fused == ([True, False, True] if topology == "fused" else [])
    # three batches, the last of another size; the plan lists are asked for one batch at a time
    asked = []

    def parts(key):
        for lo in range(0, N, B):
            asked.append((key, lo))
            yield getattr(plans.part(lo, lo + B), key)

    rows = hp.run((audio[lo:lo + B] for lo in range(0, N, B)), mixes=parts("mix"), reverbs=parts("reverb"),
                  speeds=parts("speed"), masks=parts("mask"))
    assert rows.cpu().numpy().tobytes() == want.tobytes()
    assert sorted(asked[:4]) == sorted((key, 0) for key in ("mix", "reverb", "speed", "mask")) and len(asked) == 12
    assert hp.run([audio[lo:lo + B] for lo in range(0, N, B)]).cpu().numpy().tobytes() == clean.tobytes()
