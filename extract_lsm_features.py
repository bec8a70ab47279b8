"""Stage 2 of the pipeline: spike-train dataset (File 1) -> LSM features (File 2).

Drop-in for the reference script of the same name (same CLI flags, function names, constants and
``lsm_features_larger.npz`` schema; /root/reference/extract_lsm_features.py).  The reservoir
(third-party ``snnpy`` in the reference) is ``lsm_speech_classifier_amd.snn.SNN``: all clips of a
split run through ONE batched HIP kernel launch instead of a per-clip Python loop; under
``torchrun`` the clips shard across the GPUs of the node and the feature rows are all-gathered
(RCCL).  There is no CPU fallback.
"""
import argparse
from pathlib import Path

import numpy as np

NUM_NEURONS = 1000
NUM_OUTPUT_NEURONS = 400
LEAK_COEFFICIENT = 1 / 100
REFRACTORY_PERIOD = 2
MEMBRANE_THRESHOLD = 2.0
SMALL_WORLD_P = 0.1
SMALL_WORLD_K = int(0.10 * NUM_NEURONS * 2)
WEIGHT_VARIANCE = 10
DATASET_FILE = "speech_spike_dataset_pure_redundancy.npz"
FEATURE_FILE = "lsm_features_larger.npz"
RUN_BATCH = 4096             # clips per kernel launch

_RATE = ['spike_counts', 'spike_variances', 'burst_counts']
_TIMING = ['mean_spike_times', 'first_spike_times', 'last_spike_times']
_RHYTHM = ['mean_isi', 'isi_variances']
FEATURE_SETS = {
    'all': ['spike_counts', 'spike_variances'] + _TIMING + _RHYTHM + ['burst_counts'],
    'rate': _RATE,
    'timing': _TIMING,
    'rhythm': _RHYTHM,
    'original': ['spike_counts', 'spike_variances', 'mean_spike_times'] + _RHYTHM,
}

np.random.seed(42)


def reservoir_shape(num_neurons=None, num_output_neurons=None, small_world_k=None):
    """(N, N_out, k) with the reference's constants as defaults (extract_lsm_features.py:10-16).  For another N
    the defaults follow it the way the reference's own constants relate: k = int(0.10 * N * 2) (:16) and
    N_out = 0.4 * N (400 of 1000, :10-11; the scaling BASELINE.json's larger configs use)."""
    n = NUM_NEURONS if num_neurons is None else int(num_neurons)
    if num_output_neurons is None:
        n_out = NUM_OUTPUT_NEURONS if n == NUM_NEURONS else max(1, int(0.4 * n))
    else:
        n_out = int(num_output_neurons)
    k = (SMALL_WORLD_K if n == NUM_NEURONS else int(0.10 * n * 2)) if small_world_k is None else int(small_world_k)
    if not 1 <= n_out <= n:
        raise ValueError(f"num_output_neurons={n_out} must lie in [1, num_neurons={n}]")
    return n, n_out, k


def _simulation_params(first_clip, leak_variance_divisor, num_neurons, num_output_neurons, small_world_k, seed):
    from lsm_speech_classifier_amd.snn import SimulationParams
    n, n_out, k = reservoir_shape(num_neurons, num_output_neurons, small_world_k)
    kw = {} if seed is None else {"seed": int(seed)}
    return SimulationParams(
        num_neurons=n, mean_weight=0.0, num_output_neurons=n_out,
        membrane_threshold=MEMBRANE_THRESHOLD, leak_coefficient=LEAK_COEFFICIENT,
        refractory_period=REFRACTORY_PERIOD, small_world_graph_p=SMALL_WORLD_P,
        small_world_graph_k=k, input_spike_times=first_clip,
        leak_variance_divisor=leak_variance_divisor, **kw)


def _rank0_only(rank: int):
    """Context in which only rank 0 prints: under a launcher every rank runs the same set-up lines
    (w_critico, weight, leak) and the reference's messages should appear once."""
    import contextlib
    import io
    return contextlib.nullcontext() if rank == 0 else contextlib.redirect_stdout(io.StringIO())


def calculate_theoretical_w_critico(lsm_params, input_data):
    """Mean-field critical weight from the input spike density of the first <= 500 clips:
    (theta - 2 * density * refractory) / (k / 2); 0.007 when there is no data or k == 0."""
    head = input_data[:min(500, len(input_data))]
    n_spikes = sum(int(np.sum(clip)) for clip in head)
    n_cells = sum(int(clip.shape[0]) * int(clip.shape[1]) for clip in head)
    if n_cells == 0:
        return 0.007
    density = n_spikes / n_cells
    beta = lsm_params.small_world_graph_k / 2
    if beta == 0:
        return 0.007
    w_critico = (lsm_params.membrane_threshold - 2 * density * lsm_params.refractory_period) / beta
    print(f"Theoretical w_critico: {w_critico:.8f}")
    return w_critico


def load_spike_dataset(filename=DATASET_FILE):
    if not Path(filename).exists():
        print(f"Error: Dataset not found at '{filename}'")
        return None, None
    # the reference's uint8 schema or the bit-packed one; either way the reference's arrays come back
    from lsm_speech_classifier_amd import spikefile
    X_spikes, y_labels = spikefile.load(filename)
    print(f"Loaded {len(X_spikes)} samples from '{filename}'")
    return X_spikes, y_labels


def check_time_segments(n_steps: int, time_segments: int) -> int:
    """``--time-segments K``: the clips' T steps are read in K equal segments; the segment length T // K.  K must divide T."""
    K = int(time_segments)
    if K < 1 or int(n_steps) % K != 0:
        raise ValueError(f"--time-segments {time_segments}: must be >= 1 and divide the clips' {n_steps} time steps")
    return int(n_steps) // K


def extract_all_features(lsm, spike_data, feature_keys, desc=""):
    """(n, C, T) uint8 -> (n, len(keys) * N_out) features, NaN -> 0, keys in the given order.
    Batched on the GPU (and sharded across ranks under torchrun) when ``lsm`` offers ``run_batch``;
    otherwise the reference's one-clip-at-a-time object protocol is used.  (The reference's four parameters, pinned;
    ``extract_all_segment_features`` reads the clips per time segment.)"""
    if hasattr(lsm, "run_batch"):
        import torch
        from lsm_speech_classifier_amd import dist as lsm_dist
        rank, world = lsm_dist.group_world()         # the initialised process group, else a single process
        n = len(spike_data)
        lo, hi = lsm_dist.shard_range(n, rank, world) if world > 1 else (0, n)
        if desc and rank == 0:
            print(f"{desc}: {n} clips" + (f" over {world} GPUs" if world > 1 else ""))
        rows = []
        for a in range(lo, hi, RUN_BATCH):
            batch = np.ascontiguousarray(spike_data[a:min(hi, a + RUN_BATCH)])
            # clips longer than one launch holds on chip (the plan refuses them) run as launches that hand their state on
            chunked = hasattr(lsm, "run_chunked") and batch.ndim == 3 and batch.shape[2] > lsm.max_steps(len(batch))
            feats, _, _ = (lsm.run_chunked if chunked else lsm.run_batch)(batch, feature_keys)
            rows.append(feats)
        # an empty shard still takes part in the gather: its row width comes from an empty launch-free call,
        # so it is whatever run_batch makes of these keys (unknown keys are dropped there)
        local = torch.cat(rows) if rows else lsm.run_batch(np.ascontiguousarray(spike_data[:0]), feature_keys)[0]
        return lsm_dist.gather_rows(local, n).cpu().numpy()
    rows = []
    for sample in spike_data:
        lsm.reset()
        lsm.set_input_spike_times(sample)
        lsm.simulate()
        feats = lsm.extract_features_from_spikes()
        rows.append(np.concatenate([np.nan_to_num(feats[k].copy()) for k in feature_keys if k in feats]))
    return np.array(rows)


def clip_views(spike_data, n_steps):
    """The clips of a variable-length File 1 (SPEC.md 1.14) as per-clip views ``X[b][:, :n_steps[b]]``: what
    `calculate_theoretical_w_critico`, which sums per-sample shapes, takes in place of the (n, C, T) array."""
    return [clip[:, :int(t)] for clip, t in zip(spike_data, n_steps)]


def extract_all_ragged_features(lsm, spike_data, n_steps, feature_keys, desc=""):
    """`extract_all_features` for a variable-length File 1: clip b runs its own ``n_steps[b]`` steps of the (n, C, T) rows
    (``SNN.run_batch(lengths=...)``, SPEC.md 4c; in chunks where T exceeds one launch).  One process."""
    import torch
    n = len(spike_data)
    n_steps = np.asarray(n_steps, dtype=np.int64)
    if n_steps.shape != (n,):
        raise ValueError(f"n_steps must hold one value per clip, got {n_steps.shape} for {n} clips")
    if desc:
        print(f"{desc}: {n} clips of {int(n_steps.min()) if n else 0} to {int(n_steps.max()) if n else 0} steps")
    rows = []
    for a in range(0, n, RUN_BATCH):
        batch = np.ascontiguousarray(spike_data[a:a + RUN_BATCH])
        chunked = batch.shape[2] > lsm.max_steps(len(batch))
        feats, _, _ = (lsm.run_chunked if chunked else lsm.run_batch)(batch, feature_keys, lengths=n_steps[a:a + RUN_BATCH])
        rows.append(feats)
    local = torch.cat(rows) if rows else lsm.run_batch(np.ascontiguousarray(spike_data[:0]), feature_keys)[0]
    return local.cpu().numpy()


def extract_all_segment_features(lsm, spike_data, feature_keys, desc="", time_segments=1):
    """extract_all_features per time segment: every clip is read in K = ``time_segments`` equal segments
    (``SNN.run_segments``, SPEC.md 4b) and its row is the K segment rows side by side -- (n, K * len(keys) * N_out),
    segment-major, then key-major.  The same batching, sharding and gather; K = 1 is extract_all_features itself."""
    if time_segments == 1:
        return extract_all_features(lsm, spike_data, feature_keys, desc)
    import torch
    from lsm_speech_classifier_amd import dist as lsm_dist
    if not hasattr(lsm, "run_segments"):
        raise ValueError("--time-segments needs a reservoir with run_segments (lsm_speech_classifier_amd.snn.SNN)")
    spike_data = np.asarray(spike_data)
    if spike_data.ndim != 3:
        raise ValueError(f"--time-segments needs clips of one length, got an array of shape {spike_data.shape}")
    seg = check_time_segments(spike_data.shape[2], time_segments)
    rank, world = lsm_dist.group_world()
    n = len(spike_data)
    lo, hi = lsm_dist.shard_range(n, rank, world) if world > 1 else (0, n)
    if desc and rank == 0:
        print(f"{desc}: {n} clips in {time_segments} time segments" + (f" over {world} GPUs" if world > 1 else ""))
    rows = [lsm.run_segments(np.ascontiguousarray(spike_data[a:min(hi, a + RUN_BATCH)]), seg, feature_keys)
            .reshape(min(hi, a + RUN_BATCH) - a, -1) for a in range(lo, hi, RUN_BATCH)]
    if rows:
        local = torch.cat(rows)
    else:               # an empty shard still takes part in the gather, with the row width of the others
        width = lsm.run_batch(np.ascontiguousarray(spike_data[:0]), feature_keys)[0].shape[1] * int(time_segments)
        local = torch.empty((0, width), dtype=torch.float32, device=lsm.device)
    return lsm_dist.gather_rows(local, n).cpu().numpy()


def run_network_diagnostics(lsm, X_sample_batch):
    """Health check on the first 5 clips: share of neurons that fire at least once."""
    print("\n" + "=" * 40 + "\nRUNNING NETWORK DIAGNOSTICS\n" + "=" * 40)
    n_neurons = lsm.num_neurons
    participation = []
    if hasattr(lsm, "diagnostics"):                      # one batched launch, statistics on the device
        d = lsm.diagnostics(np.ascontiguousarray(X_sample_batch[:5]))
        for i in range(len(d["participation"])):
            participation.append(float(d["participation"][i]))
            print(f"Sample {i + 1}: Active: {participation[-1]:.1f}% | Dead: {int(d['dead_neurons'][i])} | "
                  f"Avg Spikes/Neuron: {float(d['mean_spikes_per_neuron'][i]):.2f}")
        X_sample_batch = X_sample_batch[:0]
    for i, sample in enumerate(X_sample_batch[:5]):
        lsm.reset()
        lsm.set_input_spike_times(sample)
        lsm.simulate()
        spikes = getattr(lsm, "spike_matrix", None)
        if spikes is None:
            print("Warning: Cannot access internal spike matrix for diagnostics.")
            return
        per_neuron = np.sum(spikes, axis=0)
        active = int(np.count_nonzero(per_neuron))
        participation.append(active / n_neurons * 100)
        print(f"Sample {i + 1}: Active: {participation[-1]:.1f}% | Dead: {n_neurons - active} | "
              f"Avg Spikes/Neuron: {np.mean(per_neuron):.2f}")
    avg = float(np.mean(participation)) if participation else 0.0
    print("-" * 40 + f"\nDIAGNOSTIC RESULT:\n   Average Participation: {avg:.1f}%")
    if avg < 40:
        print("   STATUS: SUB-CRITICAL (Too Silent)\n   Recommendation: INCREASE multiplier or DECREASE threshold.")
    elif avg > 98:
        print("   STATUS: SUPER-CRITICAL (Epileptic/Saturated)\n   Recommendation: DECREASE multiplier.")
    else:
        print("   STATUS: EDGE OF CHAOS (Healthy)\n   (Ideal is 80-95% participation with low firing rates)")
    print("=" * 40 + "\n")
    return avg


def main_from_audio(audio, labels, n_filters: int, filterbank: str, feature_set: str, multiplier: float,
                    leak_variance_divisor: float = None, batch: int = 1024, *, num_neurons=None,
                    num_output_neurons=None, small_world_k=None, seed=None, readout=None, class_names=None,
                    time_segments=1, corrupt=None, reverb=None, speed=None, mask=None, model_out=None, epochs=1,
                    ridge_alpha=1.0, epoch_plans=None):
    """Stages 1 + 2 without File 1: audio (n, 16000) float32 + labels -> File 2, the same arrays main() writes
    after create_dataset() (tests/test_gpu_hotpath.py compares them).  The split, w_critico (first <= 500
    training clips), the reservoir and the diagnostics follow main() line by line; the features come from
    `pipeline.HotPath`: every batch of clips goes filterbank -> encoder -> reservoir on the GPU, consecutive
    batches overlapped on rotating streams, and no raster ever reaches the host.

    Under a launcher the WHOLE path shards (the clip loops of create_dataset.py:143 and
    extract_lsm_features.py:78 at once): every rank holds the clip list, encodes the same first <= 500
    training clips for w_critico (so every rank builds the same reservoir), runs its contiguous
    block of each split through its own HotPath on its own GPU, and the feature rows are all-gathered ONCE per
    split; StandardScaler and the file stay on rank 0.

    `readout` = "torch-ridge" / "torch-logistic" (the reference's host round trip is
    extract_lsm_features.py:199-212 -> train_classifier.py:27-45): the gathered rows never leave the device --
    `readout.StandardScaler` -> the PyTorch readout -> predictions, all on rank 0's GPU; File 2 is still written
    (ONE device-to-host copy of the scaled arrays, schema unchanged) and the report train_classifier.py prints is
    printed here.  Returns the test accuracy then (None otherwise, like the reference's main()).

    `time_segments` = K > 1: every clip is read in K equal time segments (`pipeline.HotPath(time_segments=K)`); File 2
    keeps its keys, the feature arrays get K times the columns.

    `corrupt` = ``(noise bank (M, L) float32, frontend.MixPlan of the n clips)``: every clip is shifted, scaled and mixed
    with noise on the GPU before its front end (SPEC.md 1.10), the clips w_critico looks at included; a rank corrupts its
    clips with their entries of the one plan.

    `reverb` = ``(bank (M, K) float32, lengths, frontend.ReverbPlan of the n clips)``: every clip is first convolved with
    its room impulse response on the GPU (SPEC.md 1.11), ahead of `corrupt`.

    `speed` = ``(factors, frontend.SpeedPlan of the n clips)``: every clip is first played at its speed among ``factors`` on
    the GPU (SPEC.md 1.12), ahead of `reverb`.

    `mask` = what `create_dataset.mask_from_args` returns: frequency bands and time spans of every clip's normalised spectrogram
    are zeroed inside the spike encoder (SPEC.md 1.13), by a plan drawn for all n clips in listing order.

    `model_out` = a path: the model file of `readout.LinearModel` (SPEC.md 6) -- with a PyTorch `readout` the whole file at
    once, otherwise its front half (scaler and parameters), which train_classifier.py --model-out completes.

    `readout` = "stream-ridge" (SPEC.md 7): no training row is kept or gathered.  The training split runs `epochs` times
    through `pipeline.fit_from_audio` into one `readout.RidgeStatistics` per rank (merged in rank order under a launcher:
    the result is that world size's, not one process's); `ridge_alpha` is the readout's penalty.  Epoch 0 uses the plans given,
    so one epoch sees exactly the rows "torch-ridge" sees; epoch e >= 1 uses ``epoch_plans(e)`` -- a dict with the `mix`,
    `reverb` and `speed` plans of all n clips drawn with the augmentation seed + e (`create_dataset.epoch_plans`) -- and the
    mask plan drawn with ``mask["seed"] + e``.  The test split is scored by `readout.DeviceReadout`; File 2 is not written,
    because no training rows exist."""
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import StandardScaler
    from lsm_speech_classifier_amd import dist as lsm_dist, frontend, pipeline
    from lsm_speech_classifier_amd.augment import AugmentChain, StepPlans
    from lsm_speech_classifier_amd.snn import SNN

    if readout not in (None, "sklearn", "torch-ridge", "torch-logistic", "stream-ridge"):
        raise ValueError(f"readout must be None, 'sklearn', 'torch-ridge', 'torch-logistic' or 'stream-ridge', got {readout!r}")
    check_stream_ridge(readout, epochs, time_segments, corrupt is not None or reverb is not None or speed is not None,
                       epoch_plans)
    on_device = readout in ("torch-ridge", "torch-logistic")
    rank, _, world = lsm_dist.init()
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int32)
    if len(audio) == 0:
        if rank == 0:
            print("Error: no audio clips")
        lsm_dist.finish()
        return
    idx_train, idx_test, y_train, y_test = train_test_split(
        np.arange(len(audio)), labels, test_size=0.2, random_state=42, stratify=labels)
    dev = lsm_dist.local_device() if world > 1 else None
    fe = frontend.SpikeFrontEnd(n_filters, filterbank, device=dev)
    check_time_segments(fe.n_steps, time_segments)                  # refused with the reason before any work is done
    check_model_out(model_out, time_segments)
    stages, plans = {}, {}
    if corrupt is not None:
        stages["mixer"], plans["mix"] = frontend.NoiseMixer(corrupt[0], device=dev), corrupt[1]
    if reverb is not None:
        stages["reverb"], plans["reverb"] = frontend.Reverberator(reverb[0], reverb[1], device=dev), reverb[2]
    if speed is not None:
        stages["speed"], plans["speed"] = frontend.SpeedPerturber(speed[0], device=dev), speed[1]
    if mask:
        plans["mask"] = frontend.mask_plan(len(audio), fe.n_filters, fe.time_bins, **mask)
    chain, plans = AugmentChain(**stages), StepPlans(**plans)
    head_plans = plans.take(idx_train[:500])
    # what w_critico and the diagnostics look at
    head = fe.encode(chain.apply(audio[idx_train[:500]], head_plans), **head_plans.mask_keyword()).cpu().numpy()
    params = _simulation_params(head[0], leak_variance_divisor, num_neurons, num_output_neurons, small_world_k, seed)
    with _rank0_only(rank):
        optimal_weight = calculate_theoretical_w_critico(params, head) * multiplier
        print(f"Using weight: {optimal_weight:.8f} (multiplier: {multiplier:.2f})")
        if leak_variance_divisor:
            print(f"Using Heterogeneous Leak. Divisor: {leak_variance_divisor}")
    params.mean_weight = optimal_weight
    params.weight_variance = WEIGHT_VARIANCE
    lsm = SNN(simulation_params=params, device=dev)
    if rank == 0:
        run_network_diagnostics(lsm, head)
    keys = FEATURE_SETS[feature_set]
    if rank == 0:
        print(f"Extracting feature set: '{feature_set}' ({len(idx_train)} + {len(idx_test)} clips, audio -> features "
              f"on the GPU" + (f", {world} ranks)" if world > 1 else ")"))

    def split_features(idx):
        """(len(idx), n_feat) float32 rows in dataset order, STILL ON THE DEVICE (every rank holds all of them)."""
        lo, hi = lsm_dist.shard_range(len(idx), rank, world)
        shard = plans.take(idx[lo:hi])
        local = pipeline.features_from_audio(audio[idx[lo:hi]], fe, lsm, keys, batch=batch, device_out=True,
                                             time_segments=time_segments,
                                             corrupt=(chain.mixer, shard.mix), reverb=(chain.reverb, shard.reverb),
                                             speed=(chain.speed, shard.speed), mask=shard.mask)
        return lsm_dist.gather_rows(local, len(idx))

    if readout == "stream-ridge":
        stats = _stream_statistics(audio, labels, idx_train, y_train, fe, lsm, keys, chain, plans, mask, batch, int(epochs),
                                   epoch_plans, rank, world)
        X_test_dev = split_features(idx_test)
        lsm_dist.finish()
        if rank != 0:
            return
        return _stream_readout(stats, X_test_dev, y_train, y_test, float(ridge_alpha), class_names, model_out,
                               pipeline.model_params(fe, params, feature_set=feature_set, multiplier=float(multiplier),
                                                     time_segments=1))
    X_train_dev = split_features(idx_train)
    X_test_dev = split_features(idx_test)
    lsm_dist.finish()
    if rank != 0:
        return
    model = None
    if model_out:
        model = dict(path=model_out, feature_keys=keys, n_out=lsm.num_output_neurons,
                     params=pipeline.model_params(fe, params, feature_set=feature_set, multiplier=float(multiplier),
                                                  time_segments=1))
    if on_device:
        return _device_readout(X_train_dev, X_test_dev, y_train, y_test, readout, feature_set,
                               leak_variance_divisor, class_names, model)
    X_train_feat, X_test_feat = X_train_dev.cpu().numpy(), X_test_dev.cpu().numpy()
    scaler = StandardScaler()
    X_train_scaled = scaler.fit_transform(X_train_feat)
    X_test_scaled = scaler.transform(X_test_feat)
    np.savez_compressed(FEATURE_FILE, X_train_features=X_train_scaled, y_train=y_train,
                        X_test_features=X_test_scaled, y_test=y_test, feature_set=feature_set,
                        leak_variance_divisor=leak_variance_divisor)
    print(f"Extraction complete. Features saved to '{FEATURE_FILE}'")
    if model:
        write_model_front(scaler, **model)


def check_stream_ridge(readout, epochs, time_segments, augmented: bool, epoch_plans) -> None:
    """The refusals of the "stream-ridge" route, made before any work is done."""
    if readout != "stream-ridge":
        if int(epochs) != 1:
            raise ValueError("epochs needs readout='stream-ridge': the other readouts keep every training row once")
        return
    if int(epochs) < 1:
        raise ValueError(f"epochs={epochs} must be >= 1")
    if int(time_segments) != 1:
        raise ValueError("readout='stream-ridge' needs time_segments = 1: the statistics hold one feature row per clip")
    if int(epochs) > 1 and augmented and epoch_plans is None:
        raise ValueError("epochs > 1 with a corruption, reverberation or speed plan needs epoch_plans: the plans of the later "
                         "epochs (create_dataset.epoch_plans)")


def _stream_statistics(audio, labels, idx_train, y_train, fe, lsm, keys, chain, plans, mask, batch, epochs, epoch_plans,
                       rank, world):
    """The training split, `epochs` times, into this rank's `RidgeStatistics`; then every rank's merged in rank order."""
    from lsm_speech_classifier_amd import dist as lsm_dist, frontend, pipeline, readout as ro
    from lsm_speech_classifier_amd.augment import StepPlans
    n_classes = int(labels.max()) + 1
    if labels.min() < 0 or n_classes > ro.MAX_CLASSES:
        raise ValueError(f"readout='stream-ridge' takes labels in [0, {ro.MAX_CLASSES}), got {int(labels.min())} to "
                         f"{int(labels.max())}")
    stats = ro.RidgeStatistics(keys, lsm.num_output_neurons, n_classes, device=lsm.device)
    lo, hi = lsm_dist.shard_range(len(idx_train), rank, world)
    for e in range(epochs):
        drawn = plans
        if e:
            later = dict(epoch_plans(e)) if epoch_plans is not None else {}
            drawn = StepPlans(later.get("speed"), later.get("reverb"), later.get("mix"),
                              frontend.mask_plan(len(audio), fe.n_filters, fe.time_bins, **dict(mask, seed=int(mask["seed"]) + e))
                              if mask else None)
            for name in ("speed", "reverb", "mix"):
                if (getattr(plans, name) is None) != (getattr(drawn, name) is None):
                    raise ValueError(f"epoch_plans({e}) must hold a {name!r} plan exactly when epoch 0 has one")
        shard = drawn.take(idx_train[lo:hi])
        pipeline.fit_from_audio(audio[idx_train[lo:hi]], y_train[lo:hi], fe, lsm, keys, stats, batch=batch,
                                corrupt=(chain.mixer, shard.mix), reverb=(chain.reverb, shard.reverb),
                                speed=(chain.speed, shard.speed), mask=shard.mask)
    return lsm_dist.merge_statistics(stats)


def _stream_readout(stats, X_test_dev, y_train, y_test, alpha, class_names, model_out, params):
    """The readout solved from the statistics, the test split scored on the device, the usual report."""
    import train_classifier as tc
    from lsm_speech_classifier_amd import readout as ro
    print(f"Solving the ridge readout from the statistics of {stats.rows} training rows on the device...")
    model = stats.to_model(alpha, tc.names_of_classes(range(stats.n_classes), class_names), params)
    scorer = ro.DeviceReadout(model, device=X_test_dev.device)
    y_pred = scorer.class_of(scorer.score_rows(X_test_dev)[1]).cpu().numpy()
    print(f"'{FEATURE_FILE}' is not written on this route: no training rows exist")
    if model_out:
        model.save(model_out)
        print(f"Model saved to '{model_out}'")
    return tc.report_results(y_train, y_test, y_pred, class_names)


def check_model_out(model_out, time_segments) -> None:
    """``--model-out`` saves a model of one SPEC.md 4 row per clip: with K > 1 time segments a row is K rows side by side,
    which the readout launches (SPEC.md 6) do not score."""
    if model_out and int(time_segments) != 1:
        raise ValueError("--model-out needs --time-segments 1: the saved model scores one feature row per clip or window")


def write_model_front(scaler, path, feature_keys, n_out, params) -> None:
    """The front half of the model file (`readout.LinearModel`): the scaler's mean and scale, the feature keys and every
    parameter the front end and the reservoir were built from.  train_classifier.py --model-out adds the readout."""
    from lsm_speech_classifier_amd import readout as ro
    ro.save_model_file(path, dict(mean=scaler.mean_, scale=scaler.scale_, feature_keys=feature_keys, n_out=n_out,
                                  params=params))
    print(f"Model front half (scaler, parameters) saved to '{path}'")


def _device_readout(X_train_dev, X_test_dev, y_train, y_test, readout, feature_set, leak_variance_divisor,
                    class_names=None, model_file=None):
    """extract_lsm_features.py:199-212 + train_classifier.py:36-52 of the reference without the host round trip:
    scaler, readout and predictions run on the tensors' device; File 2 gets the scaled arrays (one copy each)."""
    import torch
    import train_classifier as tc
    from lsm_speech_classifier_amd import readout as ro
    scaler = ro.StandardScaler()
    Xtr = scaler.fit_transform(X_train_dev)               # float32 rows in, float32 out (statistics in float64)
    Xte = scaler.transform(X_test_dev)
    ytr = torch.from_numpy(np.asarray(y_train)).to(Xtr.device)
    model = ro.RidgeReadout(1.0) if readout == "torch-ridge" else ro.LogisticReadout(1.0, 1000)
    print("Training the ridge classifier on the device..." if readout == "torch-ridge"
          else "Training the Logistic Regression classifier on the device...")
    model.fit(Xtr, ytr)
    y_pred = model.predict(Xte).cpu().numpy()
    np.savez_compressed(FEATURE_FILE, X_train_features=Xtr.cpu().numpy(), y_train=y_train,
                        X_test_features=Xte.cpu().numpy(), y_test=y_test, feature_set=feature_set,
                        leak_variance_divisor=leak_variance_divisor)
    print(f"Extraction complete. Features saved to '{FEATURE_FILE}'")
    if model_file:                                        # the whole model file at once: scaler, readout, parameters
        ro.LinearModel.from_fitted(scaler, model, model_file["feature_keys"], model_file["n_out"],
                                   tc.names_of_classes(model.classes_.cpu().numpy(), class_names),
                                   model_file["params"]).save(model_file["path"])
        print(f"Model saved to '{model_file['path']}'")
    return tc.report_results(y_train, y_test, y_pred, class_names)


def main(feature_set: str, multiplier: float, leak_variance_divisor: float = None, *, num_neurons=None,
         num_output_neurons=None, small_world_k=None, seed=None, time_segments=None, model_out=None, front_end=None):
    """The reference's three arguments; the keyword-only ones expose the module constants the reference
    hard-codes (NUM_NEURONS, NUM_OUTPUT_NEURONS, SMALL_WORLD_K, the NumPy seed), None = the reference's value.
    `time_segments` = K > 1: features per time segment, K times the columns (None or 1 = the reference's whole-clip rows).
    `model_out` = a path: the front half of the model file (`write_model_front`); File 1 does not say which front end wrote
    it, so `front_end` = ``(filterbank, n_filters)`` is needed with it."""
    time_segments = 1 if time_segments is None else int(time_segments)
    check_model_out(model_out, time_segments)
    if model_out and front_end is None:
        raise ValueError("--model-out needs --filterbank and --n-filters: File 1 does not say which front end wrote it")
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import StandardScaler
    from lsm_speech_classifier_amd import dist as lsm_dist
    from lsm_speech_classifier_amd.snn import SNN

    rank, _, world = lsm_dist.init()
    with _rank0_only(rank):
        X_spikes, y_labels = load_spike_dataset()
    if X_spikes is None:
        lsm_dist.finish()                     # every rank took this branch (same file system): leave the group together
        return
    from lsm_speech_classifier_amd import spikefile
    n_steps = spikefile.load_steps(DATASET_FILE)          # a variable-length File 1 (SPEC.md 1.14), else None
    steps_train = steps_test = None
    if n_steps is not None:
        if world > 1 or time_segments != 1:
            raise SystemExit("a variable-length dataset (key n_steps) runs in one process and without --time-segments")
        X_train, X_test, y_train, y_test, steps_train, steps_test = train_test_split(
            X_spikes, y_labels, n_steps, test_size=0.2, random_state=42, stratify=y_labels)
    else:
        X_train, X_test, y_train, y_test = train_test_split(
            X_spikes, y_labels, test_size=0.2, random_state=42, stratify=y_labels)
    if time_segments != 1:
        check_time_segments(np.asarray(X_train[0]).shape[1], time_segments)      # refused before the reservoir is built

    params = _simulation_params(X_train[0], leak_variance_divisor, num_neurons, num_output_neurons, small_world_k, seed)
    with _rank0_only(rank):
        optimal_weight = calculate_theoretical_w_critico(
            params, X_train if steps_train is None else clip_views(X_train, steps_train)) * multiplier
        print(f"Using weight: {optimal_weight:.8f} (multiplier: {multiplier:.2f})")
        if leak_variance_divisor:
            print(f"Using Heterogeneous Leak. Divisor: {leak_variance_divisor}")
    params.mean_weight = optimal_weight
    params.weight_variance = WEIGHT_VARIANCE

    lsm = SNN(simulation_params=params,       # every rank builds the same wiring (same seed)
              device=lsm_dist.local_device() if world > 1 else None)
    if rank == 0:
        run_network_diagnostics(lsm, X_train)

    keys = FEATURE_SETS[feature_set]
    if rank == 0:
        print(f"Extracting feature set: '{feature_set}'")
    if steps_train is not None:
        X_train_feat = extract_all_ragged_features(lsm, X_train, steps_train, keys, "Training")
        X_test_feat = extract_all_ragged_features(lsm, X_test, steps_test, keys, "Testing")
    elif time_segments == 1:
        X_train_feat = extract_all_features(lsm, X_train, keys, "Training")
        X_test_feat = extract_all_features(lsm, X_test, keys, "Testing")
    else:
        X_train_feat = extract_all_segment_features(lsm, X_train, keys, "Training", time_segments)
        X_test_feat = extract_all_segment_features(lsm, X_test, keys, "Testing", time_segments)
    lsm_dist.finish()
    if rank != 0:
        return

    scaler = StandardScaler()
    X_train_scaled = scaler.fit_transform(X_train_feat)
    X_test_scaled = scaler.transform(X_test_feat)
    np.savez_compressed(FEATURE_FILE, X_train_features=X_train_scaled, y_train=y_train,
                        X_test_features=X_test_scaled, y_test=y_test, feature_set=feature_set,
                        leak_variance_divisor=leak_variance_divisor)
    print(f"Extraction complete. Features saved to '{FEATURE_FILE}'")
    if model_out:
        from lsm_speech_classifier_amd import frontend, pipeline
        fe = frontend.SpikeFrontEnd(int(front_end[1]), front_end[0])
        clip = np.asarray(X_train[0])
        if fe.n_channels != clip.shape[0] or (steps_train is None and fe.n_steps != clip.shape[1]):
            raise ValueError(f"the dataset's clips are {clip.shape}, a {front_end[0]} front end of {front_end[1]} filters "
                             f"gives ({fe.n_channels}, {fe.n_steps})")
        write_model_front(scaler, model_out, keys, lsm.num_output_neurons,
                          pipeline.model_params(fe, params, feature_set=feature_set, multiplier=float(multiplier),
                                                time_segments=1))


def add_model_flags(ap):
    ap.add_argument("--model-out", type=str, default=None,
                    help="Write the front half of a model file here: scaler, feature keys and every parameter of the front "
                         "end and the reservoir (train_classifier.py --model-out adds the readout; classify.py reads it).")
    ap.add_argument("--filterbank", type=str, default=None, choices=["mel", "gammatone"],
                    help="With --model-out: the filterbank the dataset file was written with.")
    ap.add_argument("--n-filters", type=int, default=None, help="With --model-out: its number of filters.")


def add_reservoir_flags(ap):
    """extract_lsm_features.py:10-16,30 of the reference as flags (shared with main.py, which forwards them);
    defaults reproduce the reference's constants."""
    ap.add_argument("--num-neurons", type=int, default=None, help=f"Reservoir size (default {NUM_NEURONS}).")
    ap.add_argument("--num-output-neurons", type=int, default=None,
                    help=f"Read-out neurons (default {NUM_OUTPUT_NEURONS}; 0.4 * N for another N).")
    ap.add_argument("--small-world-k", type=int, default=None,
                    help="Ring neighbours of the small-world graph (default int(0.2 * N)).")
    ap.add_argument("--seed", type=int, default=None, help="Seed of the reservoir wiring (default 42).")


def add_time_segments_flag(ap):
    ap.add_argument("--time-segments", type=int, default=1,
                    help="Read every clip in K equal time segments: K feature rows per clip side by side (K must divide the "
                         "clips' time steps; default 1 = one row over the whole clip).")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Extract features from a spike train dataset using an LSM.")
    ap.add_argument("--feature-set", type=str, default="original", choices=FEATURE_SETS.keys())
    ap.add_argument("--multiplier", type=float, default=0.6)
    ap.add_argument("--leak-variance-divisor", type=float, default=None)
    add_reservoir_flags(ap)
    add_time_segments_flag(ap)
    add_model_flags(ap)
    a = ap.parse_args()
    if a.model_out and (a.filterbank is None or a.n_filters is None):
        ap.error("--model-out needs --filterbank and --n-filters: the dataset file does not say which front end wrote it")
    main(feature_set=a.feature_set, multiplier=a.multiplier, leak_variance_divisor=a.leak_variance_divisor,
         num_neurons=a.num_neurons, num_output_neurons=a.num_output_neurons, small_world_k=a.small_world_k,
         seed=a.seed, time_segments=a.time_segments, model_out=a.model_out,
         front_end=(a.filterbank, a.n_filters) if a.model_out else None)
