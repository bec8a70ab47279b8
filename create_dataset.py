"""Stage 1 of the pipeline: wav clips -> spike-train dataset (File 1).

Drop-in for the reference script of the same name (same CLI flags, function names, argument
meaning and ``speech_spike_dataset_pure_redundancy.npz`` schema; /root/reference/create_dataset.py),
with the filterbank, normalise/resize and hysteresis encoder running as HIP kernels on an MI355X
(``lsm_speech_classifier_amd.frontend``), batched over clips instead of one clip per Python
iteration.  There is no CPU fallback for those stages.
"""
import argparse
import os
import warnings
from pathlib import Path

import numpy as np

SAMPLE_RATE = 16000
DURATION = 1.0
TIME_BINS = 100
SPIKE_THRESHOLDS = [0.70, 0.80, 0.90, 0.95]
HYSTERESIS_GAP = 0.1
MAX_SAMPLES_PER_CLASS = 1000
REDUNDANCY_FACTOR = 1
COMMANDS = ["yes", "no", "up", "visual", "backward", "stop", "bird", "cat", "nine", "eight",
            "zero", "follow"]
DATASET_ROOT = Path("speech_commands_v0.02")
OUTPUT_FILE = "speech_spike_dataset_pure_redundancy.npz"
ENCODE_BATCH = 2048          # clips per GPU launch

np.random.seed(42)


def _frontend():
    from lsm_speech_classifier_amd import frontend
    return frontend


def _decode_wav(filepath: Path):
    """One PCM wav file as (rate, mono float32 at the file's own rate)."""
    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rate, data = wavfile.read(str(filepath))
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    else:
        data = data.astype(np.float32)
    if data.ndim == 2:
        data = data.mean(axis=1)
    return int(rate), data


def _one_second(data: np.ndarray) -> np.ndarray:
    want = int(SAMPLE_RATE * DURATION)
    data = data[:want]
    if len(data) < want:
        data = np.pad(data, (0, want - len(data)))
    return np.ascontiguousarray(data, dtype=np.float32)


def load_audio_file(filepath: Path):
    """One wav file as mono float32 at 16 kHz, padded/trimmed to exactly one second; None (with a
    message) when the file cannot be read.  PCM wav only (scipy.io.wavfile); other rates are
    resampled polyphase."""
    try:
        rate, data = _decode_wav(filepath)
        if rate != SAMPLE_RATE:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(rate), SAMPLE_RATE)
            data = resample_poly(data, SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
        return _one_second(data)
    except Exception as exc:
        print(f"Error loading {filepath}: {exc}")
        return None


def audio_to_spectrogram(audio: np.ndarray, n_filters: int, filterbank: str) -> np.ndarray:
    """(n_samples,) -> (n_filters, TIME_BINS) normalised spectrogram in [0, 1] (GPU)."""
    return _frontend().audio_to_spectrogram(audio, n_filters, filterbank)


def convert_spectrogram_to_spikes_hysteresis(spectrogram, thresholds, hysteresis_gap=0.05):
    """(F, n_time) -> (F, n_time * len(thresholds)) uint8, thresholds interleaved in time (GPU)."""
    return _frontend().convert_spectrogram_to_spikes_hysteresis(spectrogram, thresholds, hysteresis_gap)


def create_pure_redundancy(spike_train: np.ndarray, redundancy_factor: int) -> np.ndarray:
    return np.repeat(spike_train, redundancy_factor, axis=0)


def _list_files(commands, root: Path, per_class: int, verbose: bool = True):
    """The (wav path, label) pairs the reference's loop visits, in its order: classes in list order, the first
    `per_class` files of each folder in sorted order (create_dataset.py:130-143)."""
    listing = []
    for label, word in enumerate(commands):
        if verbose:
            print(f"Processing '{word}'...")
        folder = root / word
        if not folder.is_dir():
            if verbose:
                print(f"  Warning: Directory not found, skipping: {folder}")
            continue
        files = sorted(folder.glob("*.wav"))[:per_class]
        if not files and verbose:
            print(f"  Warning: No files found for '{word}'")
        listing += [(f, label) for f in files]
    return listing


def _load_listing(listing, kept=None):
    """``kept``, when given, receives the positions in ``listing`` of the files that could be read."""
    clips, labels = [], []
    for at, (f, label) in enumerate(listing):
        audio = load_audio_file(f)
        if audio is not None:
            clips.append(audio)
            labels.append(label)
            if kept is not None:
                kept.append(at)
    return clips, labels


def _load_listing_device(listing, device=None, kept=None):
    """`_load_listing` with the resampling on the GPU (`--resample device`): the files are decoded to mono at their own
    rates on the host, grouped by rate, every group padded with zeros to a common length and resampled in one launch
    (`frontend.Resampler`, SPEC.md 1.8).  Returns ``(clips, labels)``: a float32 (n, 16000) DEVICE tensor in listing order
    (None when nothing could be read) and the labels of its rows."""
    import torch
    fe = _frontend()
    want = int(SAMPLE_RATE * DURATION)
    decoded, labels = [], []
    for at, (f, label) in enumerate(listing):
        try:
            decoded.append(_decode_wav(f))
            labels.append(label)
            if kept is not None:
                kept.append(at)
        except Exception as exc:
            print(f"Error loading {f}: {exc}")
    if not decoded:
        return None, labels
    dev = fe.indexed_device(device)
    clips = torch.zeros((len(decoded), want), dtype=torch.float32, device=dev)
    for rate in sorted({r for r, _ in decoded}):
        rows = [i for i, (r, _) in enumerate(decoded) if r == rate]
        if rate == SAMPLE_RATE:
            group = np.stack([_one_second(decoded[i][1]) for i in rows])
            clips[torch.tensor(rows, device=dev)] = torch.from_numpy(group).to(dev)
            continue
        rs = fe.Resampler(rate, SAMPLE_RATE, device=dev)
        # an output below 16000 reads no input past rate * DURATION + Hs
        length = min(max(len(decoded[i][1]) for i in rows), int(rate * DURATION) + rs.history + 1)
        group = np.zeros((len(rows), max(length, 1)), dtype=np.float32)
        for q, i in enumerate(rows):
            x = decoded[i][1][:length]
            group[q, :len(x)] = x
        out = rs.resample(group, n_out=want)
        # resample_poly ends a clip after ceil(n * up / down) samples: what the filter's tail adds behind is dropped
        ends = torch.tensor([rs.default_length(len(decoded[i][1])) for i in rows], device=dev)
        out.masked_fill_(torch.arange(want, device=dev)[None, :] >= ends[:, None], 0.0)
        clips[torch.tensor(rows, device=dev)] = out
    return clips, labels


def _collect_audio(commands, root: Path, per_class: int):
    return _load_listing(_list_files(commands, root, per_class))


# ---- corruption on the device (SPEC.md 1.10): --noise-dir, --snr-db, --time-shift-ms, --level-db, --augment-seed --------
SYNTHETIC_NOISE_ROWS = 4
SYNTHETIC_NOISE_SECONDS = 4
DEFAULT_SNR_DB = 10.0


def load_noise_bank(noise_dir, seed: int = 42) -> np.ndarray:
    """The noise bank (M, L) float32 at 16 kHz: every wav under ``noise_dir`` in sorted order, read through `_decode_wav`
    and resampled like a clip, a shorter file repeated up to the longest one's length (the mixer wraps a row anyway);
    ``"synthetic"``: `synth.coloured_noise`.  None: one silent sample, for a shift or a level without noise."""
    if noise_dir is None:
        return np.zeros((1, 1), dtype=np.float32)
    if str(noise_dir) == "synthetic":
        from lsm_speech_classifier_amd import synth
        return synth.coloured_noise(SYNTHETIC_NOISE_ROWS, SYNTHETIC_NOISE_SECONDS * SAMPLE_RATE, seed=seed)
    rows = []
    for f in sorted(Path(noise_dir).glob("*.wav")):
        rate, data = _decode_wav(f)
        if rate != SAMPLE_RATE:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(rate), SAMPLE_RATE)
            data = resample_poly(data, SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
        if len(data):
            rows.append(np.ascontiguousarray(data, dtype=np.float32))
    if not rows:
        raise ValueError(f"--noise-dir {noise_dir}: no readable wav file")
    longest = max(len(r) for r in rows)
    return np.stack([np.resize(r, longest) for r in rows])


def corruption(augment, n_listed: int):
    """``augment`` (`augment_from_args`) -> ``(noise bank, frontend.MixPlan of all n_listed clips in listing order)``."""
    bank = load_noise_bank(augment["noise_dir"], augment["seed"])
    return bank, _mix_plan(augment, bank, n_listed, augment["seed"])


def _mix_plan(augment, bank, n_listed: int, seed: int):
    snr = augment["snr_db"] if augment["noise_dir"] is not None else np.inf
    return _frontend().mix_plan(n_listed, bank.shape[0], bank.shape[1], DEFAULT_SNR_DB if snr is None else snr,
                                max_shift=int(round(augment["time_shift_ms"] * SAMPLE_RATE / 1000.0)),
                                level_db=augment["level_db"], seed=seed)


def epoch_plans(epoch: int, n_listed: int, augment=None, corrupt=None, room=None, reverb=None, pace=None):
    """The plans of a later pass over the same n_listed clips (`extract_lsm_features.main_from_audio(epochs=...)`): what
    `corruption`, `reverberation` and `speeds` draw with --augment-seed + ``epoch``, for the banks already loaded -- ``corrupt``
    and ``reverb`` are those functions' results for epoch 0, ``augment``, ``room`` and ``pace`` the flags they were made from.
    A dict with "mix", "reverb" and "speed" for the stages in use."""
    out = {}
    if augment:
        out["mix"] = _mix_plan(augment, corrupt[0], n_listed, augment["seed"] + int(epoch))
    if room:
        out["reverb"] = _frontend().reverb_plan(n_listed, reverb[0].shape[0], prob=room["prob"], seed=room["seed"] + int(epoch))
    if pace:
        out["speed"] = _frontend().speed_plan(n_listed, len(pace["factors"]), prob=pace["prob"], seed=pace["seed"] + int(epoch))
    return out


# ---- reverberation on the device (SPEC.md 1.11): --rir-dir, --rir-prob, --rir-max-ms; the seed is --augment-seed -----------
SYNTHETIC_RIR_ROWS = 4
DEFAULT_RIR_MAX_MS = 500.0


def _cut_response(data: np.ndarray, max_taps: int):
    """One impulse response as a bank row: from its largest-magnitude sample (the direct path, so no delay is added) at
    most ``max_taps`` samples, divided in float64 by that sample's value (h[0] = 1) and rounded to float32, trailing zeros
    dropped.  None for a file without a non-zero sample."""
    data = np.asarray(data, dtype=np.float32)
    if not len(data) or not np.abs(data).max() > 0:
        return None
    at = int(np.argmax(np.abs(data)))
    h = (data[at:at + max_taps].astype(np.float64) / np.float64(data[at])).astype(np.float32)
    return h[:int(np.flatnonzero(h)[-1]) + 1]


def load_rir_bank(rir_dir, max_ms: float = DEFAULT_RIR_MAX_MS, seed: int = 42):
    """The bank of room impulse responses ``(bank (M, K) float32, lengths (M,) int32)`` at 16 kHz: every wav under
    ``rir_dir`` in sorted order, read through `_decode_wav` and resampled like a clip, cut by `_cut_response` to at most
    ``max_ms`` milliseconds and zero-padded to the longest row; ``lengths`` says where each ends.  ``"synthetic"``:
    `synth.room_responses`, cut to ``max_ms`` likewise."""
    max_taps = int(max_ms * SAMPLE_RATE / 1000.0)
    if not 1 <= max_taps <= 16384:
        raise ValueError(f"--rir-max-ms {max_ms}: a row must have 1 to 16384 taps at {SAMPLE_RATE} Hz")
    if str(rir_dir) == "synthetic":
        from lsm_speech_classifier_amd import synth
        bank, lengths = synth.room_responses(SYNTHETIC_RIR_ROWS, seed=seed)
        rows = [bank[r, :n] for r, n in enumerate(lengths)]
    else:
        rows = []
        for f in sorted(Path(rir_dir).glob("*.wav")):
            rate, data = _decode_wav(f)
            if rate != SAMPLE_RATE:
                from math import gcd
                from scipy.signal import resample_poly
                g = gcd(int(rate), SAMPLE_RATE)
                data = resample_poly(data, SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
            rows.append(data)
    rows = [h for h in (_cut_response(r, max_taps) for r in rows) if h is not None]
    if not rows:
        raise ValueError(f"--rir-dir {rir_dir}: no readable wav file with a non-zero sample")
    lengths = np.array([len(h) for h in rows], dtype=np.int32)
    bank = np.zeros((len(rows), int(lengths.max())), dtype=np.float32)
    for r, h in enumerate(rows):
        bank[r, :len(h)] = h
    return bank, lengths


def reverberation(reverb, n_listed: int):
    """``reverb`` (`reverb_from_args`) -> ``(bank, lengths, frontend.ReverbPlan of all n_listed clips in listing order)``."""
    bank, lengths = load_rir_bank(reverb["rir_dir"], reverb["max_ms"], reverb["seed"])
    return bank, lengths, _frontend().reverb_plan(n_listed, bank.shape[0], prob=reverb["prob"], seed=reverb["seed"])


# ---- masks inside the spike encoder (SPEC.md 1.13): --freq-masks, --freq-mask-width, --time-masks, --time-mask-width,
# ---- --mask-prob; the seed is --augment-seed
def masks(mask, n_listed: int, fe):
    """``mask`` (`mask_from_args`) -> the frontend.MaskPlan of all n_listed clips in listing order, for front end ``fe``."""
    try:
        return _frontend().mask_plan(n_listed, fe.n_filters, fe.time_bins, **mask)
    except ValueError as e:
        raise SystemExit(f"mask flags: {e}")


# ---- speed perturbation on the device (SPEC.md 1.12): --speed-factors, --speed-prob; the seed is --augment-seed ---------------
def speeds(speed, n_listed: int):
    """``speed`` (`speed_from_args`) -> ``(factors, frontend.SpeedPlan of all n_listed clips in listing order)``."""
    factors = list(speed["factors"])
    return factors, _frontend().speed_plan(n_listed, len(factors), prob=speed["prob"], seed=speed["seed"])


def _synthetic_audio(commands, per_class: int):
    from lsm_speech_classifier_amd import synth
    labels = np.repeat(np.arange(len(commands)), per_class)
    return list(synth.class_chirps(labels, seed=1234)), list(labels)


def read_commands_file(path) -> list:
    """One class name per line (blank lines and #-comments skipped)."""
    with open(path) as fh:
        return [ln.strip() for ln in fh if ln.strip() and not ln.lstrip().startswith("#")]


def collect_audio(commands=None, dataset_root=None, max_per_class: int = MAX_SAMPLES_PER_CLASS,
                  synthetic_per_class: int = 0):
    """The clips create_dataset() would encode, as arrays: (n, 16000) float32 and int32 labels (label =
    position in the class list) -- the entry of the in-memory route (extract_lsm_features.main_from_audio),
    which skips File 1.  Empty arrays when nothing could be read."""
    commands = list(COMMANDS if commands is None else commands)
    root = Path(DATASET_ROOT if dataset_root is None else dataset_root)
    if synthetic_per_class > 0:
        clips, labels = _synthetic_audio(commands, synthetic_per_class)
    else:
        clips, labels = _collect_audio(commands, root, max_per_class)
    if not clips:
        return np.zeros((0, int(SAMPLE_RATE * DURATION)), dtype=np.float32), np.zeros(0, dtype=np.int32)
    return np.stack(clips).astype(np.float32, copy=False), np.asarray(labels, dtype=np.int32)


# ---- utterances of their own lengths (SPEC.md 1.14): --variable-length, --max-seconds ----------------------------------------
BINS_PER_SECOND = 100        # one time bin per 160 samples, the reference's TIME_BINS / DURATION
MIN_UTTERANCE_SAMPLES = 321  # three time bins: the shortest clip the ragged front end takes


def load_utterance_file(filepath: Path, max_seconds: float = DURATION):
    """One wav file as mono float32 at 16 kHz at its OWN length: not padded to a second, trimmed at ``max_seconds``, and
    zero-padded only where it is shorter than three time bins; None (with a message) when the file cannot be read."""
    try:
        rate, data = _decode_wav(filepath)
        if rate != SAMPLE_RATE:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(rate), SAMPLE_RATE)
            data = resample_poly(data, SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
        data = np.ascontiguousarray(data[:max_bins_of(max_seconds) * (SAMPLE_RATE // BINS_PER_SECOND)], dtype=np.float32)
        if len(data) < MIN_UTTERANCE_SAMPLES:
            data = np.pad(data, (0, MIN_UTTERANCE_SAMPLES - len(data)))
        return data
    except Exception as exc:
        print(f"Error loading {filepath}: {exc}")
        return None


def max_bins_of(max_seconds: float) -> int:
    bins = int(round(float(max_seconds) * BINS_PER_SECOND))
    if bins < 3:
        raise SystemExit(f"--max-seconds {max_seconds}: a clip has at least 3 time bins of 10 ms")
    return bins


def _synthetic_utterances(commands, per_class: int, max_bins: int):
    """The synthetic corpus cut to seeded lengths between 0.3 and 1.0 of the longest clip (one second at most)."""
    clips, labels = _synthetic_audio(commands, per_class)
    hop = SAMPLE_RATE // BINS_PER_SECOND
    top = min(max_bins * hop, int(SAMPLE_RATE * DURATION))
    lengths = np.random.RandomState(4321).randint(max(MIN_UTTERANCE_SAMPLES, int(0.3 * top)), top + 1, size=len(clips))
    return [np.ascontiguousarray(c[:n]) for c, n in zip(clips, lengths)], labels


def create_variable_length_dataset(n_filters: int, filterbank: str, commands=None, dataset_root=None,
                                   max_per_class: int = MAX_SAMPLES_PER_CLASS, synthetic_per_class: int = 0,
                                   output_file: str = OUTPUT_FILE, max_seconds: float = DURATION, trim=None, augment=None,
                                   reverb=None, mask=None, speed=None):
    """File 1 with every clip at its own length (`--variable-length`, SPEC.md 1.14): the wav files are not padded to one
    second, only trimmed at ``max_seconds``, and go through the ragged front end (`SpikeFrontEnd.encode_ragged`) in batches,
    longest first.  ``X_spikes`` keeps its schema at the stride ``100 * max_seconds * n_thr`` steps -- clip r's rows hold its
    ``n_steps[r]`` steps and zeros behind them -- and the file gains the key ``n_steps`` (n,) int32, which
    extract_lsm_features.py hands to the reservoir as the clips' lengths.  One process.  ``trim``
    (`trim_from_args`): every clip is first cut to its speech on the GPU (`frontend.SilenceTrimmer`, SPEC.md 1.15), so the
    rows hold the trimmed clips and ``n_steps`` their lengths.  ``reverb`` (`reverb_from_args`), ``augment``
    (`augment_from_args`) and ``mask`` (`mask_from_args`): behind the trim every clip is reverberated, mixed with noise and
    masked inside the encoder at its OWN length (SPEC.md 1.16; `AugmentChain.apply_ragged`, `frontend.mask_plan_ragged`), from
    plans drawn for the whole listing in listing order.  ``speed`` (`speed_from_args`): ahead of the trim every clip is played
    at a speed drawn from a list of factors, as the clip alone (SPEC.md 1.18; `AugmentChain.speed_ragged`), from
    `speeds` for the whole listing in listing order; the rows hold the perturbed (then trimmed) clips and ``n_steps`` their
    lengths, a slowed clip cut at ``max_seconds``."""
    from lsm_speech_classifier_amd import spikefile
    commands = list(COMMANDS if commands is None else commands)
    root = Path(DATASET_ROOT if dataset_root is None else dataset_root)
    max_bins = max_bins_of(max_seconds)
    print(f"Creating variable-length dataset with filterbank: {filterbank}, filters: {n_filters}, up to {max_bins} time bins")
    if synthetic_per_class > 0:
        clips, labels = _synthetic_utterances(commands, synthetic_per_class, max_bins)
    else:
        clips, labels = [], []
        for f, label in _list_files(commands, root, max_per_class):
            audio = load_utterance_file(f, max_seconds)
            if audio is not None:
                clips.append(audio)
                labels.append(label)
    if not clips:
        print("\nERROR: No audio files were successfully processed.")
        return
    fr = _frontend()
    fe = fr.SpikeFrontEnd(n_filters, filterbank, redundancy=REDUNDANCY_FACTOR, thresholds=SPIKE_THRESHOLDS,
                          gap=HYSTERESIS_GAP, time_bins=max_bins, n_samples=max_bins * fr.RAGGED_HOP)
    audio, bins = fr.pack_utterances(clips, max_bins)
    X = np.zeros((len(clips), fe.n_channels, fe.n_steps), dtype=np.uint8)
    from lsm_speech_classifier_amd.augment import AugmentChain, StepPlans
    samples = None
    if speed:
        import torch
        factors, paces = speeds(speed, len(clips))
        pace = AugmentChain(speed=fr.SpeedPerturber(factors, device=fe.device))
        lengths = bins.astype(np.int64) * fr.RAGGED_HOP
        new_bins = -(-fr.speed_ragged_lengths(lengths, paces.choice, pace.speed, fe.n_samples) // fr.RAGGED_HOP)
        if (new_bins < fr.RAGGED_MIN_BINS).any():
            r = int(np.nonzero(new_bins < fr.RAGGED_MIN_BINS)[0][0])
            raise SystemExit(f"--speed-factors: clip {r} of the listing has {int(bins[r])} time bins and {int(new_bins[r])} at "
                             f"speed {factors[int(paces.choice[r])]}: a clip needs {fr.RAGGED_MIN_BINS}")
        rows = torch.empty((len(clips), fe.n_samples), dtype=torch.float32, device=fe.device)
        samples = torch.empty((len(clips),), dtype=torch.int32, device=fe.device)
        for a in range(0, len(clips), ENCODE_BATCH):
            _, part, _ = pace.speed_ragged(audio[a:a + ENCODE_BATCH], lengths[a:a + ENCODE_BATCH],
                                           StepPlans(speed=paces.part(a, a + ENCODE_BATCH)), time_bins=max_bins,
                                           out=rows[a:a + ENCODE_BATCH])
            samples[a:a + ENCODE_BATCH] = part
        audio, bins = rows, new_bins.astype(np.int32)   # the host bins from the formula: nothing is read back
        print(f"  Speeds {','.join(map(str, factors))}: {int(bins.min())} / {float(bins.mean()):.1f} / {int(bins.max())} time bins "
              f"(min / mean / max)")
    if trim:
        import torch
        trimmer = fr.SilenceTrimmer(device=fe.device, **trim)
        rows = torch.empty((len(clips), fe.n_samples), dtype=torch.float32, device=fe.device)
        kept = torch.empty((len(clips),), dtype=torch.int32, device=fe.device)
        for a in range(0, len(clips), ENCODE_BATCH):
            given = bins[a:a + ENCODE_BATCH].astype(np.int64) * fr.RAGGED_HOP if samples is None else samples[a:a + ENCODE_BATCH]
            _, part, _ = trimmer.trim(audio[a:a + ENCODE_BATCH], given, time_bins=max_bins, out=rows[a:a + ENCODE_BATCH])
            kept[a:a + ENCODE_BATCH] = part
        audio, bins = rows, kept.cpu().numpy()          # the one read-back: the order below and n_steps need host values
        print(f"  Trimmed at {trim['top_db']:g} dB: {int(bins.min())} / {float(bins.mean()):.1f} / {int(bins.max())} time bins "
              f"(min / mean / max)")
    plans, stages = {}, {}
    if augment:
        bank, plans["mix"] = corruption(augment, len(clips))
        stages["mixer"] = fr.NoiseMixer(bank, device=fe.device)
    if reverb:
        rir, rir_lengths, plans["reverb"] = reverberation(reverb, len(clips))
        stages["reverb"] = fr.Reverberator(rir, rir_lengths, device=fe.device)
    if mask:
        try:
            plans["mask"] = fr.mask_plan_ragged(bins, fe.n_filters, fe.time_bins, **mask)
        except ValueError as e:
            raise SystemExit(f"mask flags: {e}")
    chain, plans = AugmentChain(**stages), StepPlans(**plans)
    order = np.argsort(-bins.astype(np.int64), kind="stable")
    for a in range(0, len(order), ENCODE_BATCH):
        idx = order[a:a + ENCODE_BATCH]
        step = plans.take(idx)
        x = chain.apply_ragged(audio[idx], bins[idx].astype(np.int64) * fr.RAGGED_HOP, step)
        raster, _ = fe.encode_ragged(x, bins[idx], **step.mask_keyword())
        X[idx] = raster.cpu().numpy()
    n_steps = (bins.astype(np.int64) * len(SPIKE_THRESHOLDS)).astype(np.int32)
    print("\nDataset created successfully.")
    print(f"  Shape: {X.shape}, clips of {int(n_steps.min())} to {int(n_steps.max())} steps")
    print(f"  Avg spikes per sample: {int(X.sum(dtype=np.int64)) / len(X):.1f}")
    spikefile.save(output_file, X_spikes=X, y_labels=np.asarray(labels, dtype=np.int32), n_steps=n_steps)
    print(f"Saved to '{output_file}'")


def create_dataset(n_filters: int, filterbank: str, commands=None, dataset_root=None,
                   max_per_class: int = MAX_SAMPLES_PER_CLASS, synthetic_per_class: int = 0,
                   output_file: str = OUTPUT_FILE, packed: bool = False, resample: str = "host", augment=None,
                   reverb=None, speed=None, mask=None):
    """Build File 1.  The first two arguments are the reference's; the keyword arguments expose
    what the reference hard-codes (class list, corpus folder, per-class cap) plus a synthetic
    corpus for machines without Speech Commands.  ``packed=True`` writes the bit-packed schema of
    ``lsm_speech_classifier_amd.spikefile`` (rasters packed on the GPU, 8x fewer bytes off the
    device and on disk); the default is the reference's uint8 schema.  ``resample="device"`` resamples files that are not
    at 16 kHz on the GPU (`_load_listing_device`) instead of one by one on the host.  ``augment`` (`augment_from_args`):
    every clip is shifted, scaled and mixed with noise on the GPU before the front end (SPEC.md 1.10), by a plan drawn for
    the whole listing in listing order -- a shard takes its slice, so any number of ranks writes the same bytes.
    ``reverb`` (`reverb_from_args`): every clip is first convolved on the GPU with a room impulse response (SPEC.md 1.11),
    by a plan drawn for the whole listing likewise.  ``speed`` (`speed_from_args`): ahead of both, every clip is played at a
    speed drawn from a list of factors on the GPU (SPEC.md 1.12) and padded or trimmed to the clip length.  ``mask``
    (`mask_from_args`): frequency bands and time spans of every clip's normalised spectrogram are zeroed inside the spike
    encoder (SPEC.md 1.13), by a plan drawn for the whole listing likewise.

    Under a launcher (torchrun: RANK / WORLD_SIZE) the clip loop of create_dataset.py:143 shards: rank r reads
    and encodes the r-th contiguous block of the file listing on its own GPU, the raster blocks are all-gathered
    in rank order (= the single-process order) and rank 0 writes the file -- the same bytes as one process."""
    if resample not in ("host", "device"):
        raise ValueError(f"resample must be 'host' or 'device', got {resample!r}")
    from lsm_speech_classifier_amd import dist as lsm_dist
    rank, _, world = lsm_dist.init()
    commands = list(COMMANDS if commands is None else commands)
    root = Path(DATASET_ROOT if dataset_root is None else dataset_root)
    if rank == 0:
        print(f"Creating dataset with filterbank: {filterbank}, filters: {n_filters}"
              + (f" ({world} ranks)" if world > 1 else ""))
    planned = bool(augment) or bool(reverb) or bool(speed) or bool(mask)
    kept = [] if planned else None          # positions in the shard's part of the listing of the clips that were read
    if synthetic_per_class > 0:
        clips, labels = _synthetic_audio(commands, synthetic_per_class)
        n_listed = len(clips)
        lo, hi = lsm_dist.shard_range(len(clips), rank, world)
        clips, labels = clips[lo:hi], labels[lo:hi]
        kept = list(range(hi - lo)) if planned else None
    else:
        listing = _list_files(commands, root, max_per_class, verbose=rank == 0)
        n_listed = len(listing)
        lo, hi = lsm_dist.shard_range(len(listing), rank, world)
        if resample == "device":
            clips, labels = _load_listing_device(listing[lo:hi], lsm_dist.local_device() if world > 1 else None, kept)
            clips = [] if clips is None else clips
        else:
            clips, labels = _load_listing(listing[lo:hi], kept)
    if not len(clips) and world == 1:
        print("\nERROR: No audio files were successfully processed.")
        return

    import torch
    dev = lsm_dist.local_device() if world > 1 else None
    fe = _frontend().SpikeFrontEnd(n_filters, filterbank, device=dev, redundancy=REDUNDANCY_FACTOR,
                                   thresholds=SPIKE_THRESHOLDS, gap=HYSTERESIS_GAP,
                                   time_bins=TIME_BINS, n_samples=int(SAMPLE_RATE * DURATION))
    from lsm_speech_classifier_amd import spikefile
    from lsm_speech_classifier_amd.augment import AugmentChain, StepPlans
    stages, plans = {}, {}
    if augment:
        bank, plans["mix"] = corruption(augment, n_listed)
        stages["mixer"] = _frontend().NoiseMixer(bank, device=dev)
    if reverb:
        rir, rir_lengths, plans["reverb"] = reverberation(reverb, n_listed)
        stages["reverb"] = _frontend().Reverberator(rir, rir_lengths, device=dev)
    if speed:
        factors, plans["speed"] = speeds(speed, n_listed)
        stages["speed"] = _frontend().SpeedPerturber(factors, device=dev)
    if mask:
        plans["mask"] = masks(mask, n_listed, fe)
    chain, plans = AugmentChain(**stages), StepPlans(**plans)
    if planned:
        plans = plans.take(lo + np.asarray(kept, dtype=np.int64))
    parts, n_spikes = [], 0
    for a in range(0, len(clips), ENCODE_BATCH):
        batch = clips[a:a + ENCODE_BATCH]
        if not torch.is_tensor(batch):
            batch = np.stack(batch)
        step = plans.part(a, a + ENCODE_BATCH)
        raster = fe.encode(chain.apply(batch, step), **step.mask_keyword())
        n_spikes += int(raster.count_nonzero())
        part = _frontend().pack_raster(raster) if packed else raster
        parts.append(part if world > 1 else part.cpu().numpy())
    if world > 1:
        # one exchange: every rank's rows (device, flattened) and labels, in rank order
        width = fe.n_channels * ((fe.n_steps + 7) // 8 if packed else fe.n_steps)
        local = (torch.cat(parts).reshape(len(clips), width) if parts
                 else torch.empty((0, width), dtype=torch.uint8, device=fe.device))
        rows = lsm_dist.gather_varrows(local)
        y_all = lsm_dist.gather_varrows(torch.tensor(labels, dtype=torch.int32, device=fe.device).reshape(-1, 1))
        tot = lsm_dist.gather_varrows(torch.tensor([[n_spikes]], dtype=torch.int64, device=fe.device))
        lsm_dist.finish()
        if rank != 0:
            return
        if rows.shape[0] == 0:
            print("\nERROR: No audio files were successfully processed.")
            return
        X = rows.cpu().numpy().reshape(rows.shape[0], fe.n_channels, -1)
        y_labels = y_all.cpu().numpy().reshape(-1).astype(np.int32)
        n_spikes = int(tot.sum())
    else:
        X = np.concatenate(parts).astype(np.uint8, copy=False)
        y_labels = np.asarray(labels, dtype=np.int32)

    print("\nDataset created successfully.")
    print(f"  Shape: {(len(X), fe.n_channels, fe.n_steps)}" + (" (bit-packed on disk)" if packed else ""))
    print(f"  Avg spikes per sample: {n_spikes / len(X):.1f}")
    if packed:
        spikefile.save(output_file, packed=X, time_steps=fe.n_steps, y_labels=y_labels)
    else:
        spikefile.save(output_file, X_spikes=X, y_labels=y_labels)
    print(f"Saved to '{output_file}'")


def add_corpus_flags(ap):
    """What the reference hard-codes at create_dataset.py:15,108-120 as flags, defaults = the reference's values
    (shared with main.py, which forwards them)."""
    ap.add_argument("--commands", type=str, default=None,
                    help="Comma-separated class list (default: the reference's 12 words).")
    ap.add_argument("--commands-file", type=str, default=None, help="File with one class name per line.")
    ap.add_argument("--dataset-root", type=str, default=None,
                    help=f"Corpus folder with one sub-folder per class (default: {DATASET_ROOT}).")
    ap.add_argument("--max-per-class", type=int, default=MAX_SAMPLES_PER_CLASS,
                    help="Per-class cap on the sorted file list.")
    ap.add_argument("--synthetic-per-class", type=int,
                    default=int(os.environ.get("LSM_SYNTHETIC_PER_CLASS", "0")),
                    help="Generate this many synthetic clips per class instead of reading wav files.")


def _number_or_range(text, flag):
    """"A" or "A,B" -> a float or a (lo, hi) tuple."""
    try:
        values = [float(v) for v in str(text).split(",")]
    except ValueError:
        values = []
    if len(values) not in (1, 2):
        raise SystemExit(f"{flag} takes a number or two separated by a comma, got {text!r}")
    return values[0] if len(values) == 1 else (min(values), max(values))


def add_augment_flags(ap):
    """The corruption flags (shared with main.py, which forwards them).  Without any of them nothing changes."""
    ap.add_argument("--noise-dir", type=str, default=None,
                    help="Folder of background-noise wav files mixed into every clip on the GPU, or 'synthetic'.")
    ap.add_argument("--snr-db", type=str, default=None,
                    help=f"Signal-to-noise ratio in dB, A or a range A,B drawn per clip (default {DEFAULT_SNR_DB:g}).")
    ap.add_argument("--time-shift-ms", type=float, default=0.0,
                    help="Shift every clip by up to this many milliseconds either way, zero filled.")
    ap.add_argument("--level-db", type=str, default=None, help="Level change in dB, A or a range A,B drawn per clip.")
    ap.add_argument("--augment-seed", type=int, default=42, help="Seed of the per-clip draws.")


def augment_from_args(a):
    """None when no corruption flag is given, else what create_dataset(augment=...) takes."""
    if a.noise_dir is None and not a.time_shift_ms and a.level_db is None:
        if a.snr_db is not None:
            raise SystemExit("--snr-db needs --noise-dir")
        return None
    if a.time_shift_ms < 0:
        raise SystemExit("--time-shift-ms must be >= 0")
    return dict(noise_dir=a.noise_dir, snr_db=None if a.snr_db is None else _number_or_range(a.snr_db, "--snr-db"),
                time_shift_ms=float(a.time_shift_ms),
                level_db=0.0 if a.level_db is None else _number_or_range(a.level_db, "--level-db"), seed=int(a.augment_seed))


def add_reverb_flags(ap):
    """The reverberation flags (shared with main.py, which forwards them).  Without --rir-dir nothing changes.  The seed of
    the per-clip draws is --augment-seed (`add_augment_flags`)."""
    ap.add_argument("--rir-dir", type=str, default=None,
                    help="Folder of room-impulse-response wav files convolved with every clip on the GPU, or 'synthetic'.")
    ap.add_argument("--rir-prob", type=float, default=1.0, help="Share of the clips that are reverberated (default 1).")
    ap.add_argument("--rir-max-ms", type=float, default=DEFAULT_RIR_MAX_MS,
                    help=f"Cut every response to this many milliseconds (default {DEFAULT_RIR_MAX_MS:g}).")


def reverb_from_args(a):
    """None without --rir-dir, else what create_dataset(reverb=...) takes."""
    if a.rir_dir is None:
        return None
    if not 0.0 <= a.rir_prob <= 1.0:
        raise SystemExit("--rir-prob must lie in [0, 1]")
    if not a.rir_max_ms > 0:
        raise SystemExit("--rir-max-ms must be > 0")
    return dict(rir_dir=a.rir_dir, prob=float(a.rir_prob), max_ms=float(a.rir_max_ms), seed=int(a.augment_seed))


def add_mask_flags(ap):
    """The mask flags (shared with main.py, which forwards them).  Without a mask count and width nothing changes.  The seed
    of the per-clip draws is --augment-seed (`add_augment_flags`)."""
    ap.add_argument("--freq-masks", type=int, default=0, help="Frequency bands zeroed per clip inside the encoder (default 0).")
    ap.add_argument("--freq-mask-width", type=int, default=0, help="Largest width of a frequency band, in filters.")
    ap.add_argument("--time-masks", type=int, default=0, help="Time spans zeroed per clip inside the encoder (default 0).")
    ap.add_argument("--time-mask-width", type=int, default=0, help="Largest width of a time span, in time bins.")
    ap.add_argument("--mask-prob", type=float, default=1.0, help="Share of the clips that are masked (default 1).")


def mask_from_args(a):
    """None unless a kind of mask has both a count and a width, else what create_dataset(mask=...) takes."""
    for flag, v in (("--freq-masks", a.freq_masks), ("--freq-mask-width", a.freq_mask_width), ("--time-masks", a.time_masks),
                    ("--time-mask-width", a.time_mask_width)):
        if v < 0:
            raise SystemExit(f"{flag} must be >= 0")
    if not 0.0 <= a.mask_prob <= 1.0:
        raise SystemExit("--mask-prob must lie in [0, 1]")
    if not (a.freq_masks and a.freq_mask_width) and not (a.time_masks and a.time_mask_width):
        return None
    return dict(freq_masks=int(a.freq_masks), freq_width=int(a.freq_mask_width), time_masks=int(a.time_masks),
                time_width=int(a.time_mask_width), prob=float(a.mask_prob), seed=int(a.augment_seed))


def add_speed_flags(ap):
    """The speed flags (shared with main.py, which forwards them).  Without --speed-factors nothing changes.  The seed of the
    per-clip draws is --augment-seed (`add_augment_flags`)."""
    ap.add_argument("--speed-factors", type=str, default=None,
                    help="Comma-separated playback speeds drawn per clip on the GPU, e.g. 0.9,1.0,1.1 (each in [0.5, 2]).")
    ap.add_argument("--speed-prob", type=float, default=1.0, help="Share of the clips whose speed is drawn (default 1).")


def speed_from_args(a):
    """None without --speed-factors, else what create_dataset(speed=...) takes."""
    if a.speed_factors is None:
        return None
    if not 0.0 <= a.speed_prob <= 1.0:
        raise SystemExit("--speed-prob must lie in [0, 1]")
    factors = [w.strip() for w in str(a.speed_factors).split(",") if w.strip()]
    try:
        tables, _ = _frontend().speed_bank(factors)
    except ValueError as e:
        raise SystemExit(f"--speed-factors {a.speed_factors}: {e}")
    if not tables:
        raise SystemExit(f"--speed-factors {a.speed_factors}: every factor is 1, there is nothing to perturb")
    return dict(factors=factors, prob=float(a.speed_prob), seed=int(a.augment_seed))


def add_variable_length_flags(ap):
    """The variable-length flags (shared with main.py, which forwards them).  Without --variable-length nothing changes."""
    ap.add_argument("--variable-length", action="store_true",
                    help="Keep every clip at its own length (ragged front end) instead of padding it to one second; File 1 "
                         "gains the key n_steps.")
    ap.add_argument("--max-seconds", type=float, default=DURATION,
                    help=f"With --variable-length: trim clips at this many seconds (default {DURATION:g}); sets the row stride.")
    ap.add_argument("--trim-silence", type=float, default=None, metavar="DB",
                    help="With --variable-length: cut every clip on the GPU to the 10 ms bins within DB decibels of its loudest "
                         "one; File 1's n_steps are the trimmed lengths.")
    ap.add_argument("--trim-pad-ms", type=float, default=DEFAULT_TRIM_PAD_MS,
                    help=f"With --trim-silence: keep this much around the speech, in whole bins (default {DEFAULT_TRIM_PAD_MS:g}).")
    ap.add_argument("--trim-min-ms", type=float, default=DEFAULT_TRIM_MIN_MS,
                    help=f"With --trim-silence: the shortest a trimmed clip gets, in whole bins (default {DEFAULT_TRIM_MIN_MS:g}).")
    ap.add_argument("--augment-variable-length", action="store_true",
                    help="With --variable-length: let the corruption flags, --rir-dir and the mask flags through -- every clip is "
                         "reverberated, mixed and masked at its own (trimmed) length (SPEC.md 1.16).")
    ap.add_argument("--speed-variable-length", action="store_true",
                    help="With --variable-length --augment-variable-length: let --speed-factors / --speed-prob through -- every "
                         "clip is first played at its speed, alone, and File 1's n_steps are the perturbed (then trimmed) "
                         "lengths (SPEC.md 1.18).")


DEFAULT_TRIM_PAD_MS = 30.0
DEFAULT_TRIM_MIN_MS = 30.0       # three time bins: the shortest clip the ragged front end takes


def trim_from_args(a):
    """None without --trim-silence, else what create_variable_length_dataset(trim=...) takes: top_db, pad_bins, min_bins."""
    if getattr(a, "trim_silence", None) is None:
        return None
    if not a.variable_length:
        raise SystemExit("--trim-silence needs --variable-length: a trimmed clip has a length of its own")
    if not (np.isfinite(a.trim_silence) and a.trim_silence > 0):
        raise SystemExit("--trim-silence must be a number of dB above 0")
    if not a.trim_pad_ms >= 0:
        raise SystemExit("--trim-pad-ms must be >= 0")
    ms_per_bin = 1000.0 / BINS_PER_SECOND
    min_bins = int(round(a.trim_min_ms / ms_per_bin))
    if not 3 <= min_bins <= max_bins_of(a.max_seconds):
        raise SystemExit(f"--trim-min-ms {a.trim_min_ms:g}: a trimmed clip has 3 to {max_bins_of(a.max_seconds)} time bins of 10 ms")
    return dict(top_db=float(a.trim_silence), pad_bins=int(round(a.trim_pad_ms / ms_per_bin)), min_bins=min_bins)


def check_variable_length_args(a):
    """--variable-length is a route of its own: refuse the flags it does not take instead of ignoring them.  Only with
    --augment-variable-length does it take the corruption flags, --rir-dir and the mask flags (SPEC.md 1.16), and only with
    --speed-variable-length beside that flag the speed flags (SPEC.md 1.18)."""
    max_bins_of(a.max_seconds)
    refused = not getattr(a, "augment_variable_length", False)      # the three flag groups of the augmentation chain
    no_speed = refused or not getattr(a, "speed_variable_length", False)
    taken = [flag for flag, on in (("--packed", getattr(a, "packed", False)), ("--resample device", getattr(a, "resample", "host") == "device"),
                                   ("the corruption flags", refused and augment_from_args(a) is not None),
                                   ("--rir-dir", refused and reverb_from_args(a) is not None), ("--speed-factors", no_speed and a.speed_factors is not None),
                                   ("the mask flags", refused and mask_from_args(a) is not None)) if on]
    if taken:
        raise SystemExit(f"--variable-length does not combine with {', '.join(taken)}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--variable-length runs in one process")


def commands_from_args(a):
    if a.commands_file:
        return read_commands_file(a.commands_file)
    if a.commands:
        return [w.strip() for w in a.commands.split(",") if w.strip()]
    return None


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Create a spike train dataset from audio files.")
    ap.add_argument("--n-filters", type=int, default=128, help="Number of filters for the filterbank.")
    ap.add_argument("--filterbank", type=str, default="gammatone", choices=["mel", "gammatone"],
                    help="Type of filterbank to use.")
    add_corpus_flags(ap)
    ap.add_argument("--packed", action="store_true",
                    default=os.environ.get("LSM_PACKED_DATASET", "0") == "1",
                    help="Write the bit-packed File 1 schema (8x fewer raster bytes).")
    ap.add_argument("--resample", type=str, default="host", choices=["host", "device"],
                    help="Where files that are not at 16 kHz are resampled: one by one on the host (default), or grouped by "
                         "rate on the GPU.")
    add_augment_flags(ap)
    add_reverb_flags(ap)
    add_speed_flags(ap)
    add_mask_flags(ap)
    add_variable_length_flags(ap)
    a = ap.parse_args()
    trim = trim_from_args(a)
    if a.variable_length:
        check_variable_length_args(a)
        create_variable_length_dataset(n_filters=a.n_filters, filterbank=a.filterbank, commands=commands_from_args(a),
                                       dataset_root=a.dataset_root, max_per_class=a.max_per_class,
                                       synthetic_per_class=a.synthetic_per_class, max_seconds=a.max_seconds, trim=trim,
                                       **({"augment": augment_from_args(a), "reverb": reverb_from_args(a),
                                           "mask": mask_from_args(a)} if a.augment_variable_length else {}),
                                       **({"speed": speed_from_args(a)}
                                          if a.augment_variable_length and a.speed_variable_length else {}))
        raise SystemExit(0)
    create_dataset(n_filters=a.n_filters, filterbank=a.filterbank, commands=commands_from_args(a),
                   dataset_root=a.dataset_root, max_per_class=a.max_per_class,
                   synthetic_per_class=a.synthetic_per_class, packed=a.packed, resample=a.resample,
                   augment=augment_from_args(a), reverb=reverb_from_args(a), speed=speed_from_args(a),
                   mask=mask_from_args(a))
