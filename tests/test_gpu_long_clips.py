"""Clips longer than one launch holds on chip, and recordings taken window by window (SPEC.md 4a).

A launch keeps the whole clip's input bits in LDS, 4 * ceil(C / 32) bytes per step: with 2000 channels a reservoir of
1024 neurons is refused beyond a few hundred steps (tests/test_gpu_envelope.py pins that the LDS bounds the steps, not
the ABI).  `SNN.run_chunked` serves such a clip in launches that hand their state on, and
`pipeline.features_from_long_audio` carries the state of a liquid from one window of a recording to the next.  The
reference is the plain-C oracle on the WHOLE raster, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _last_accepted_steps(net, n_clips):
    """Largest n_steps in [1, 65535] that plan(n_clips, n_steps, 0) accepts, by asking plan (as test_gpu_envelope.py)."""
    from lsm_speech_classifier_amd import _lib

    def accepted(t):
        try:
            net.plan(n_clips, t, 0)
            return True
        except _lib.LsmHipError as e:
            assert "layout" in str(e), str(e)
            return False
    lo, hi = 1, 65536
    assert accepted(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    return lo


def test_clip_longer_than_a_launch_holds(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, reservoir as R, snn, synth
    n, k, n_out, c, b = 1024, 24, 64, 2000, 2
    res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                               mean_weight=0.3, refractory_period=2), c)
    net = snn.SNN(None, reservoir=res)
    t_max = _last_accepted_steps(net, b)
    assert t_max < 1000, t_max
    assert net.max_steps(b) == t_max                                  # lsm_reservoir_max_steps is that number
    t = 2 * t_max + 17
    rasters = synth.bernoulli_raster(b, c, t, 0.05, seed=7)
    ref = []
    for r in rasters:
        f, sm, _ = oracle_c.lif_run(res, r, ALL_KEYS)
        per = sm.sum(axis=0, dtype=np.int64)
        ref.append((f, sm, [int(np.count_nonzero(per)), int(per.sum())]))
        # every launch has spikes to hand on and to count
        assert per.sum() > 10 * t and sm[t_max - 1].any() and sm[2 * t_max - 1].any() and sm[2 * t_max:].any()
    # the one-launch path refuses it, as before
    with pytest.raises(_lib.LsmHipError, match="layout"):
        net.run_batch(rasters, ALL_KEYS)
    chunks = snn.split_steps(t, t_max)
    assert len(chunks) == 3 and [n_ for _, n_ in chunks] == [t_max, t_max, 17]
    assert chunks[0][0] == 0 and all(a[0] + a[1] == b_[0] for a, b_ in zip(chunks, chunks[1:])) and sum(chunks[-1]) == t
    stats = torch.full((b, 2), -1, dtype=torch.int32, device="cuda")
    f, sm, vt = net.run_chunked(rasters, ALL_KEYS, want_spike_matrix=True, stats_out=stats)
    assert vt is None and tuple(sm.shape) == (b, t, n)
    f, sm, stats = f.cpu().numpy(), sm.cpu().numpy(), stats.cpu().numpy()
    for i, (f_ref, sm_ref, st_ref) in enumerate(ref):
        np.testing.assert_array_equal(sm[i], sm_ref, err_msg=f"spike matrix, clip {i}")
        np.testing.assert_array_equal(f[i], f_ref, err_msg=f"features, clip {i}")
        assert stats[i].tolist() == st_ref, f"statistics, clip {i}"
    # a chunk length of the caller's own
    f2, _, _ = net.run_chunked(rasters, ALL_KEYS, chunk_steps=400)
    np.testing.assert_array_equal(f2.cpu().numpy(), f)


def test_recording_window_by_window(torch_cuda, oracle_c):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
    n_rec, windows = 2, 3
    fe = frontend.SpikeFrontEnd(16, "gammatone")
    steps = fe.n_steps
    assert steps * windows == 1200
    res = R.build_reservoir(R.SimulationParams(num_neurons=256, num_output_neurons=100, small_world_graph_k=50,
                                               mean_weight=2.0 / 25, refractory_period=2), fe.n_channels)
    net = snn.SNN(None, reservoir=res)
    clips = synth.class_chirps([0, 5, 9, 3, 7, 11], seed=31)                      # (6, n_samples): two recordings of three
    audio = np.ascontiguousarray(clips.reshape(n_rec, windows * clips.shape[1]))
    # the GPU front end (checked against the oracle in its own tests), window by window: the per-clip normalisation
    rasters = fe.encode(torch.from_numpy(clips).cuda()).cpu().numpy().reshape(n_rec, windows, fe.n_channels, steps)
    whole = np.concatenate([rasters[:, w] for w in range(windows)], axis=2)      # (n_rec, C, 1200)
    assert whole.shape == (n_rec, fe.n_channels, 1200)

    carried = pipeline.features_from_long_audio(audio, fe, net, ALL_KEYS).cpu().numpy()
    alone = pipeline.features_from_long_audio(audio, fe, net, ALL_KEYS, carry_state=False).cpu().numpy()
    assert carried.shape == alone.shape == (n_rec, windows, 8 * 100)
    for i in range(n_rec):
        sm_whole = oracle_c.lif_run(res, whole[i], ALL_KEYS)[1]
        for w in range(windows):
            prefix = np.ascontiguousarray(whole[i][:, :steps * (w + 1)])
            np.testing.assert_array_equal(carried[i, w], oracle_c.lif_run(res, prefix, ALL_KEYS)[0],
                                          err_msg=f"recording {i}, windows 0..{w} carried")
            f_alone, sm_alone, _ = oracle_c.lif_run(res, rasters[i, w], ALL_KEYS)
            np.testing.assert_array_equal(alone[i, w], f_alone, err_msg=f"recording {i}, window {w} from reset")
            if w == 1:
                # the liquid remembers: the second window from the carried state is not the second window from reset
                assert sm_alone.any() and not np.array_equal(sm_whole[steps:2 * steps], sm_alone), \
                    f"recording {i}: the inputs are too quiet to show a carried state"
    for w in range(windows):
        independent, _, _ = net.run_batch(np.ascontiguousarray(rasters[:, w]), ALL_KEYS)
        np.testing.assert_array_equal(alone[:, w], independent.cpu().numpy(), err_msg=f"window {w}: carry_state=False")
    assert not np.array_equal(carried[:, 1], alone[:, 1])
