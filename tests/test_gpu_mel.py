"""Mel branch on the GPU vs the NumPy restatement of librosa's defaults (oracle/ref_numpy.py).
Floating point with an FFT inside: the tolerance is stated per quantity; everything after the dB
array (normalise, resize, encoder) is bit-exact on identical input (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = [0.70, 0.80, 0.90, 0.95]


def _audio(n, seed):
    from lsm_speech_classifier_amd import synth
    a = synth.class_chirps(list(range(n)), seed=seed)
    a[n // 2:] = synth.white_noise(n - n // 2, seed=seed + 1)
    return a


@pytest.mark.parametrize("n_mels", [13, 40, 80, 128])
def test_mel_frontend_matches_oracle(n_mels):
    import torch
    from lsm_speech_classifier_amd import frontend
    from oracle import ref_numpy as O
    audio = _audio(4, seed=n_mels)
    fe = frontend.SpikeFrontEnd(n_mels, "mel")
    assert fe.ncols == 101 and fe._mel.hop == 160
    dev = torch.from_numpy(audio).cuda()
    power = fe._mel.power(dev).cpu().numpy()
    db, _ = fe.spectrogram_db(audio)
    raster, norm = fe.spikes_from_db(db, want_norm=True)
    db, norm, raster = db.cpu().numpy(), norm.cpu().numpy(), raster.cpu().numpy()
    assert db.dtype == np.float32 and db.shape == (4, n_mels, 101)
    flips = 0
    for b in range(4):
        p_ref = O.mel_power(audio[b], n_mels)
        # float64 FFT on both sides, float32 power and projection
        np.testing.assert_allclose(power[b], p_ref, rtol=1e-5, atol=2e-6 * p_ref.max())   # measured 2e-7
        d_ref = O.power_to_db(p_ref)
        np.testing.assert_allclose(db[b], d_ref, rtol=0, atol=1e-4)          # dB; measured 6e-6
        n_ref = O.normalise_resize(d_ref)
        np.testing.assert_allclose(norm[b], n_ref, rtol=0, atol=5e-6)       # measured 2.4e-7
        # the encoder on the GPU's own normalised spectrogram is exact ...
        np.testing.assert_array_equal(raster[b], O.encode_hysteresis(norm[b], THR, 0.1))
        # ... and against the oracle's raster only threshold ties may flip
        flips += int((raster[b] != O.encode_hysteresis(n_ref, THR, 0.1)).sum())
    assert flips == 0                                    # (larger seeded set: test_mel_rasters_equal_the_oracle_exactly)


@pytest.mark.parametrize("n_samples,time_bins", [(15999, 100), (8001, 100), (1500, 100), (4097, 37), (2048, 64), (333, 10)])
def test_mel_power_over_clip_lengths(n_samples, time_bins):
    """Clips whose length is odd, not a multiple of the hop, or SHORTER than the 2048-sample window (every frame then reaches
    past both ends of the clip), odd hops: the frame's samples come from clamped indices and are dropped where the frame lies
    outside the clip (csrc/mel.hip) -- against the oracle's zero-padded frames, power and dB within SPEC.md 1.5's tolerances,
    both routes giving the same raster."""
    import torch
    from lsm_speech_classifier_amd import frontend, synth
    from oracle import ref_numpy as O
    full = synth.class_chirps([0, 3, 7], seed=n_samples)
    audio = np.ascontiguousarray(full[:, :n_samples])
    audio[2] = synth.white_noise(1, seed=n_samples + 1)[0, :n_samples]
    fe = frontend.SpikeFrontEnd(24, "mel", time_bins=time_bins, n_samples=n_samples)
    hop = max(1, int(n_samples / time_bins))
    assert fe._mel.hop == hop and fe.ncols == 1 + n_samples // hop
    power = fe._mel.power(torch.from_numpy(audio).cuda()).cpu().numpy()
    db, _ = fe.spectrogram_db(audio)
    for b in range(3):
        p_ref = O.mel_power(audio[b], 24, hop=hop)
        assert p_ref.shape == power[b].shape
        np.testing.assert_allclose(power[b], p_ref, rtol=1e-5, atol=2e-6 * p_ref.max())
        np.testing.assert_allclose(db[b].cpu().numpy(), O.power_to_db(p_ref), rtol=0, atol=1e-4)
    assert torch.equal(fe.encode(audio, fused=False), fe.encode(audio, fused=True))


@pytest.mark.parametrize("n_mels", [13, 40, 80, 128])
def test_mel_rasters_equal_the_oracle_exactly(n_mels):
    """the mel branch's rasters are asserted EQUAL to the oracle's (create_dataset.py:43-48 + :62-98 through
    oracle/ref_numpy.py), not within a flip budget: 64 seeded clips per filter count -- chirps, white noise, a faded and a
    very quiet clip.  The power spectrogram differs from the oracle's at the 1e-7 level (own float64 FFT, SPEC.md 1.5); a
    raster byte could only differ where a normalised value lies within that distance of a threshold, and none of these
    102 400 x 4 values per filter count does.  Both routes (one launch, three launches)."""
    from lsm_speech_classifier_amd import frontend, synth
    from oracle import ref_numpy as O
    n = 64
    audio = synth.class_chirps(np.arange(n) % 12, seed=1000 + n_mels)
    audio[n // 2:] = synth.white_noise(n - n // 2, seed=2000 + n_mels)
    audio[5] *= np.linspace(1.0, 0.0, audio.shape[1], dtype=np.float32)
    audio[40] *= 1e-4
    fe = frontend.SpikeFrontEnd(n_mels, "mel")
    ref = np.stack([O.encode_hysteresis(O.normalise_resize(O.mel_db(a, n_mels)), THR, 0.1) for a in audio])
    assert ref.any(axis=(1, 2)).all()
    for kw in (dict(fused=False), dict(fused=True)):
        got = fe.encode(audio, **kw).cpu().numpy()
        flips = int((got != ref).sum())
        assert flips == 0, (kw, flips)


def test_cfg1_shape_end_to_end(oracle_c):
    """BASELINE.json configs[0] shape: 40 mel filters, 500-neuron reservoir, through both stages;
    the reservoir part must equal the oracle bit for bit on the GPU's own rasters."""
    from lsm_speech_classifier_amd import frontend, reservoir as R, snn, synth
    from oracle import ref_numpy as O
    audio = synth.class_chirps(np.arange(8) % 4, seed=3)
    rasters = frontend.SpikeFrontEnd(40, "mel").encode(audio).cpu().numpy()
    assert rasters.shape == (8, 40, 400) and rasters.any()
    p = R.SimulationParams(num_neurons=500, num_output_neurons=200, small_world_graph_k=100)
    p.mean_weight = O.w_critico(100, 2.0, 2, rasters) * 0.6
    res = R.build_reservoir(p, 40)
    net = snn.SNN(p, reservoir=res)
    feats, _, _ = net.run_batch(rasters, ["spike_counts", "mean_isi", "burst_counts"])
    ref = oracle_c.lif_run_batch(res, rasters, ["spike_counts", "mean_isi", "burst_counts"], n_threads=8)
    np.testing.assert_array_equal(feats.cpu().numpy(), ref)


def test_audio_to_spectrogram_mel_single_clip():
    from lsm_speech_classifier_amd import frontend
    from oracle import ref_numpy as O
    audio = _audio(2, seed=9)[0]
    out = frontend.audio_to_spectrogram(audio, 40, "mel")
    assert out.shape == (40, 100) and out.dtype == np.float32
    np.testing.assert_allclose(out, O.normalise_resize(O.mel_db(audio, 40)), rtol=0, atol=5e-5)


@pytest.mark.parametrize("n_mels,redundancy,thr,gap", [(40, 1, THR, 0.1), (128, 1, THR, 0.1), (13, 2, [0.5, 0.9], 0.05),
                                                       (200, 1, [0.3, 0.6, 0.65, 0.7, 0.8, 0.9, 0.95, 0.99], 0.02)])
def test_one_launch_mel_front_end_equals_the_three_launch_route(n_mels, redundancy, thr, gap):
    """Round 4: `lsm_mel_spikes_f32` -- mel power, power_to_db, normalise, resize, encoder in one launch,
    the workgroup that finishes a clip's last frame finishing the clip -- gives the rasters of the split route
    (`lsm_mel_power_f32` -> `lsm_power_to_db_f32` -> `lsm_spec_to_spikes_f32`) bit for bit: batches of 1..9 clips, a silent
    clip, repeated launches on one workspace (the arrival counters are left zeroed), 1-8 thresholds, row repeat.
    Reference: /root/reference/create_dataset.py:43-48, 62-104."""
    import torch
    from lsm_speech_classifier_amd import frontend
    fe = frontend.SpikeFrontEnd(n_mels, "mel", redundancy=redundancy, thresholds=thr, gap=gap)
    assert not fe.will_fuse()                              # measured slower than the split launches: opt-in
    audio = _audio(9, seed=n_mels)
    audio[3] = 0.0
    dev = torch.from_numpy(audio).cuda()
    split = fe.encode(dev)
    assert torch.equal(split, fe.encode(dev, fused=False))
    for rep in range(3):                                   # the same cached workspace every time
        fused = fe.encode(dev, fused=True)
        assert fused.shape == (9, n_mels * redundancy, 100 * len(thr)) and torch.equal(fused, split), rep
    assert split.any() and not split[3].any()
    for n in (1, 2, 5):
        assert torch.equal(fe.encode(dev[:n], fused=True), split[:n])
    big = torch.from_numpy(np.resize(audio, (140, audio.shape[1]))).cuda()     # >= 128 clips: one workgroup per clip
    assert torch.equal(fe.encode(big, fused=True), fe.encode(big, fused=False))
    ws = fe.new_workspace(9)
    out = torch.empty_like(split)
    assert fe.encode(dev, fused=True, raster_out=out, workspace=ws) is out and torch.equal(out, split)
    torch.cuda.synchronize()
    assert not ws[:9 * 4].any()                            # counters back at zero
    with pytest.raises(ValueError):
        fe.encode(dev, fused=True, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))


def test_mel_shapes_too_long_for_one_launch_take_the_split_route(monkeypatch):
    """The one-launch kernel's finishing workgroup keeps its latch bit rows (64 rows x thresholds x time-bin words, twice) in
    the 68 KB of its waves' point buffers: 1200 time bins x 4 thresholds do not fit, any number of filters does."""
    import torch
    from lsm_speech_classifier_amd import frontend, synth
    monkeypatch.setenv("LSM_MEL_ONE_LAUNCH", "1")
    audio = synth.class_chirps([0, 4], seed=5)
    fe = frontend.SpikeFrontEnd(24, "mel", time_bins=1200)
    assert not fe.will_fuse()                               # even when asked for
    r = fe.encode(audio)                                    # split route, silently
    assert r.shape == (2, 24, 4800) and r.any()
    with pytest.raises(ValueError):
        fe.encode(audio, fused=True)
    wide = frontend.SpikeFrontEnd(700, "mel")
    assert wide.will_fuse()
    r1, r2 = wide.encode(audio), wide.encode(audio, fused=False)
    assert r1.shape == (2, 700, 400) and r1.any() and torch.equal(r1, r2)


@pytest.mark.parametrize("one_launch", [True, False])
def test_hotpath_with_the_mel_front_end_equals_the_serial_path(monkeypatch, one_launch):
    """cfg1's shape through the overlapped pipeline on both mel routes.  One launch (LSM_MEL_ONE_LAUNCH=1): front ends on
    streams of their own, each with its OWN workspace (two launches sharing the arrival counters would finish each other's
    clips); split launches (the default): rasters from the allocator, handed over with record_stream.  Rows equal to the
    serial path either way."""
    import torch
    if one_launch:
        monkeypatch.setenv("LSM_MEL_ONE_LAUNCH", "1")
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn, synth
    from oracle import ref_numpy as O
    keys = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']
    audio = synth.class_chirps(np.arange(6 * 50) % 4, seed=11)
    fe = frontend.SpikeFrontEnd(40, "mel")
    rasters = fe.encode(audio, fused=False)
    p = R.SimulationParams(num_neurons=500, num_output_neurons=200, small_world_graph_k=100,
                           mean_weight=O.w_critico(100, 2.0, 2, rasters.cpu().numpy()) * 0.6)
    net = snn.SNN(None, reservoir=R.build_reservoir(p, 40))
    serial, _, _ = net.run_batch(rasters, keys)
    batches = [torch.from_numpy(audio[lo:lo + 50]).cuda() for lo in range(0, len(audio), 50)]
    for streams, fes in ((1, None), (4, 0), (6, None)):
        hp = pipeline.HotPath(fe, net, keys, streams=streams, fe_streams=fes)
        for rep in range(3):
            assert torch.equal(hp.run(batches), serial), (streams, fes, rep)
    assert fe.will_fuse() == one_launch
    if one_launch:
        assert len({ring.workspace.data_ptr() for ring in hp._rasters.values()}) == len(hp._rasters) >= 2
    else:
        assert not hp._rasters
