"""The one-launch step (`lsm_step_fused_f64`, include/lsm_hip_step.h): the lane-pair gammatone front end and the dense-row
reservoir of a clip in one workgroup, against the two launches it replaces (`net.run_batch(fe.encode(x))`) and the C oracle,
bit for bit; what `lsm_step_fused_supported` refuses; and `pipeline.HotPath`, which takes the launch with at most 4 hardware
queues."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(97, 256), (97, 1000), (128, 256), (128, 1000)]      # F = 97: ragged last 32-channel group; N = 256: 1 slot per lane
SILENT, NAN, LOUD = 1, 2, 3                                    # positions of the special clips in the batch of five
_cases = {}


def _clips():
    from lsm_speech_classifier_amd import synth
    audio = np.concatenate([synth.class_chirps([0, 5, 7], seed=31), synth.white_noise(1, seed=9),
                            synth.class_chirps([9], seed=4)])
    audio[SILENT] = 0.0                                        # flat spectrogram: no input spike
    audio[NAN, 7000] = np.nan                                  # NaN max / min: an all-zero raster
    return np.ascontiguousarray(audio, dtype=np.float32)


def _case(F, N):
    """Front end, reservoir, the five clips on the device and what the two launches give for them (computed once)."""
    if (F, N) not in _cases:
        import torch
        from lsm_speech_classifier_amd import frontend, reservoir as R, snn
        from oracle import ref_numpy as O
        audio = _clips()
        fe = frontend.SpikeFrontEnd(F, "gammatone")
        rasters = fe.encode(audio)
        k = N // 5
        wc = O.w_critico(k, 2.0, 2, rasters[[0, 4]].cpu().numpy())
        p = R.SimulationParams(num_neurons=N, num_output_neurons=2 * N // 5, small_world_graph_k=k, mean_weight=wc * 1.0)
        net = snn.SNN(None, reservoir=R.build_reservoir(p, F))
        stats = torch.zeros((len(audio), 2), dtype=torch.int32, device="cuda")
        feats = net.run_batch(rasters, stats_out=stats, waves_per_clip=-1)[0]
        torch.cuda.synchronize()
        _cases[(F, N)] = dict(fe=fe, net=net, audio=torch.from_numpy(audio).cuda(), rasters=rasters.cpu().numpy(),
                              feats=feats.clone(), stats=stats.clone())
    return _cases[(F, N)]


@pytest.mark.parametrize("F,N", SHAPES)
def test_fused_step_equals_the_two_launches(F, N):
    """Batches of 1, 3 and 5 clips (silent, NaN and loud clips among them), every feature set and stats_out."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    from lsm_speech_classifier_amd.snn import FEATURE_KEYS
    c = _case(F, N)
    fe, net = c["fe"], c["net"]
    assert not c["rasters"][SILENT].any() and not c["rasters"][NAN].any() and c["rasters"][LOUD].any()
    for B in (1, 3, 5):
        assert pipeline.step_fused_supported(fe, net, B)
        stats = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
        got = pipeline.step_fused(fe, net, c["audio"][:B], stats_out=stats)
        torch.cuda.synchronize()
        assert got.shape == (B, len(FEATURE_KEYS) * net.num_output_neurons)
        assert torch.equal(got, c["feats"][:B]), f"B={B}: rows differ from run_batch(encode(x))"
        assert torch.equal(stats, c["stats"][:B]), f"B={B}: stats_out differs"
    # a subset of the keys in another order, into a caller's buffer
    keys = ["isi_variances", "spike_counts", "mean_spike_times"]
    out = torch.empty((5, 3 * net.num_output_neurons), dtype=torch.float32, device="cuda")
    assert pipeline.step_fused(fe, net, c["audio"], keys, features_out=out) is out
    assert torch.equal(out, net.run_batch(torch.from_numpy(c["rasters"]).cuda(), keys)[0])
    assert float(c["feats"][LOUD].abs().sum()) > 0 and int(c["stats"][LOUD, 1]) > int(c["stats"][0, 1])


@pytest.mark.parametrize("F,N", SHAPES)
def test_fused_step_equals_the_oracle(oracle_c, F, N):
    """Three clips through the C oracle, front end and reservoir; the loud clip takes the merge path of the spike exchange:
    some producer wave of the 4-wave layout has more than its 16 fixed list slots of spikes in one step."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    c = _case(F, N)
    fe, net = c["fe"], c["net"]
    coefs = fe.coefs.cpu().numpy()
    audio = c["audio"].cpu().numpy()
    got = pipeline.step_fused(fe, net, c["audio"]).cpu().numpy()
    per_wave = max(64, -(-N // 4))
    for b in (0, NAN, LOUD):
        with np.errstate(all="ignore"):
            raster = oracle_c.encode_hysteresis(oracle_c.normalise_resize(oracle_c.gammatone_db(
                oracle_c.gammatone_spec(audio[b], coefs, fe.nwin, fe.hop, fe.ncols)), fe.time_bins), fe.thresholds, fe.gap)
        np.testing.assert_array_equal(raster, c["rasters"][b])
        feats, sm, _ = oracle_c.lif_run(net.reservoir, raster)
        np.testing.assert_array_equal(got[b], feats.reshape(-1))
        if b == LOUD:
            sl = 1
            while sl * 64 < per_wave:
                sl *= 2
            assert max(int(sm[:, w * sl * 64:(w + 1) * sl * 64].sum(axis=1).max()) for w in range(4)) > 16


def test_unsupported_shapes_are_refused_and_take_the_two_launches(monkeypatch):
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, pipeline, reservoir as R, snn
    c = _case(128, 1000)
    fe, net, audio = c["fe"], c["net"], c["audio"]
    nets = {}

    def net_for(channels, **kw):
        if (channels, tuple(kw.items())) not in nets:
            p = R.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=200,
                                   mean_weight=0.01, **kw)
            nets[(channels, tuple(kw.items()))] = snn.SNN(None, reservoir=R.build_reservoir(p, channels))
        return nets[(channels, tuple(kw.items()))]

    refused = {
        "64 filters: 2 groups of 32 channels": (frontend.SpikeFrontEnd(64, "gammatone"), net_for(64)),
        "96 filters: 3 groups": (frontend.SpikeFrontEnd(96, "gammatone"), net_for(96)),
        "redundancy 2: 256 channels": (frontend.SpikeFrontEnd(128, "gammatone", redundancy=2), net_for(256)),
        "mel front end": (frontend.SpikeFrontEnd(128, "mel"), net),
        "refractory period 3": (fe, net_for(128, refractory_period=3)),
        "4 live windows": (frontend.SpikeFrontEnd(128, "gammatone", n_samples=12000), net),
    }
    for why, (f, n) in refused.items():
        assert not pipeline.step_fused_supported(f, n, 5), why
    net.set_kernel("sparse")
    try:
        assert not pipeline.step_fused_supported(fe, net, 5), "sparse kernel"
        with pytest.raises(_lib.LsmHipError):
            pipeline.step_fused(fe, net, audio)
    finally:
        net.set_kernel("auto")
    assert pipeline.step_fused_supported(fe, net, 5)
    # HotPath with 4 hardware queues: the fused launch where it is served, the two launches everywhere else
    monkeypatch.setattr(pipeline, "configure_hardware_queues", lambda n=12: 4)
    calls = []
    real = pipeline.step_fused
    monkeypatch.setattr(pipeline, "step_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    hp = pipeline.HotPath(fe, net, streams=6)
    assert hp.fused_step and hp.n_fused_streams == 3
    rows, _ = hp.submit(audio)
    hp.synchronize()
    assert len(calls) == 1 and torch.equal(rows, c["feats"])
    f96, n96 = refused["96 filters: 3 groups"]
    hp96 = pipeline.HotPath(f96, n96, streams=6)
    assert hp96.fused_step                                     # 4 queues: asked for, but the library does not serve the shape
    rows96, _ = hp96.submit(audio)
    hp96.synchronize()
    assert len(calls) == 1 and torch.equal(rows96, n96.run_batch(f96.encode(audio))[0])
    assert not pipeline.HotPath(fe, net, streams=6, time_segments=2).fused_step
    assert not pipeline.HotPath(fe, net, streams=1).fused_step
    # a masked step, a front-end-only and a reservoir-only step of the served shape keep their launches too
    hp.submit(audio, stage="frontend")
    hp.submit(torch.from_numpy(c["rasters"]).cuda(), stage="reservoir")
    hp.submit(audio, mask=frontend.mask_plan(5, fe.n_filters, fe.time_bins, freq_masks=1, freq_width=8))
    hp.synchronize()
    assert len(calls) == 1
    # more than 4 queues: nothing changes
    monkeypatch.setattr(pipeline, "configure_hardware_queues", lambda n=12: 12)
    hp12 = pipeline.HotPath(fe, net, streams=6)
    assert not hp12.fused_step
    rows12, _ = hp12.submit(audio)
    hp12.synchronize()
    assert len(calls) == 1 and torch.equal(rows12, c["feats"])


_CHILD = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
from oracle import ref_numpy as O
assert os.environ["GPU_MAX_HW_QUEUES"] == "4"
audio = synth.class_chirps(np.arange(7 * 24) % 12, seed=77)
fe = frontend.SpikeFrontEnd(128, "gammatone")
rasters = fe.encode(audio)
p = R.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=200,
                       mean_weight=O.w_critico(200, 2.0, 2, rasters.cpu().numpy()) * 0.6)
net = snn.SNN(None, reservoir=R.build_reservoir(p, 128))
keys = ["spike_counts", "mean_isi", "isi_variances"]
serial = net.run_batch(rasters, keys)[0]
calls = []
real = pipeline.step_fused
pipeline.step_fused = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
hp = pipeline.HotPath(fe, net, keys, time_reservoir=True)
assert hp.hw_queues == 4 and hp.fused_step and hp.n_fused_streams == 3
rows = hp.run([audio[i * 24:(i + 1) * 24] for i in range(7)])
assert len(calls) == 7 and len(hp.reservoir_events) == 7
assert all(a.elapsed_time(b) > 0 for a, b in hp.reservoir_events)
assert torch.equal(rows, serial)
print("child ok", int(rows.sum().item()))
"""


def test_hotpath_with_four_queues_in_a_child_process():
    """A fresh process with GPU_MAX_HW_QUEUES=4: HotPath.run over 7 batches makes 7 fused launches, rows = the serial path's."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "child ok" in p.stdout


def test_fused_step_in_a_graph():
    """One capture of the fused launch on a single stream, replayed on new audio in the captured buffer."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    c = _case(128, 1000)
    fe, net = c["fe"], c["net"]
    x = c["audio"][[4, 0, 3]].clone()
    out = torch.zeros((3, 8 * net.num_output_neurons), dtype=torch.float32, device="cuda")
    ws = fe.new_workspace(3)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        pipeline.step_fused(fe, net, x, features_out=out, workspace=ws)       # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            pipeline.step_fused(fe, net, x, features_out=out, workspace=ws)
    torch.cuda.synchronize()
    x.copy_(c["audio"][[0, 3, 4]])
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, c["feats"][[0, 3, 4]])
