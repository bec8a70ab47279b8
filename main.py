"""Run the three pipeline stages in order, each as its own Python process (like the reference's
main.py, which shells out and ignores exit codes: /root/reference/main.py:19-27).

Beyond the reference's four flags, the constants it hard-codes in the stage scripts are flags here too and are
forwarded to the stages (defaults = the reference's values, so `python main.py` is unchanged): the class list,
corpus folder and per-class cap of stage 1 (create_dataset.py:15,108-120), the reservoir shape and seed of
stage 2 (extract_lsm_features.py:10-16,30), the readout of stage 3.  `--nproc N` starts stages 1 and 2 (or the
in-memory route) as N ranks, one per GPU, through torch.distributed.run; the readout stays one process."""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))     # the stage scripts live next to this file;
                                                      # data files stay relative to the working directory


def _corpus_args(a):
    out = []
    if a.commands:
        out += ["--commands", a.commands]
    if a.commands_file:
        out += ["--commands-file", a.commands_file]
    if a.dataset_root:
        out += ["--dataset-root", a.dataset_root]
    if a.max_per_class is not None:
        out += ["--max-per-class", str(a.max_per_class)]
    if a.synthetic_per_class:
        out += ["--synthetic-per-class", str(a.synthetic_per_class)]
    return out


def _augment_args(a):
    out = []
    for flag, v in (("--noise-dir", a.noise_dir), ("--snr-db", a.snr_db), ("--level-db", a.level_db)):
        if v is not None:
            out += [flag, str(v)]
    if a.time_shift_ms:
        out += ["--time-shift-ms", str(a.time_shift_ms)]
    if out:
        out += ["--augment-seed", str(a.augment_seed)]
    return out


def _reverb_args(a):
    """Nothing without --rir-dir; the seed goes along unless the corruption flags already carry it."""
    if a.rir_dir is None:
        return []
    out = ["--rir-dir", str(a.rir_dir), "--rir-prob", str(a.rir_prob), "--rir-max-ms", str(a.rir_max_ms)]
    return out if _augment_args(a) else out + ["--augment-seed", str(a.augment_seed)]


def _speed_args(a):
    """Nothing without --speed-factors; the seed goes along unless the corruption or reverberation flags already carry it."""
    if a.speed_factors is None:
        return []
    out = ["--speed-factors", str(a.speed_factors), "--speed-prob", str(a.speed_prob)]
    return out if _augment_args(a) or _reverb_args(a) else out + ["--augment-seed", str(a.augment_seed)]


def _mask_args(a):
    """Nothing unless a kind of mask has a count and a width; the seed goes along unless other flags already carry it."""
    if not (a.freq_masks and a.freq_mask_width) and not (a.time_masks and a.time_mask_width):
        return []
    out = ["--freq-masks", str(a.freq_masks), "--freq-mask-width", str(a.freq_mask_width), "--time-masks", str(a.time_masks),
           "--time-mask-width", str(a.time_mask_width), "--mask-prob", str(a.mask_prob)]
    return out if _augment_args(a) or _reverb_args(a) or _speed_args(a) else out + ["--augment-seed", str(a.augment_seed)]


def _variable_length_args(a):
    """Nothing without --variable-length; the trim flags go along with --trim-silence, --augment-variable-length and
    --speed-variable-length where given."""
    if not a.variable_length:
        return []
    out = ["--variable-length", "--max-seconds", str(a.max_seconds)]
    if getattr(a, "augment_variable_length", False):
        out += ["--augment-variable-length"]
    if getattr(a, "speed_variable_length", False):
        out += ["--speed-variable-length"]
    if a.trim_silence is not None:
        out += ["--trim-silence", str(a.trim_silence), "--trim-pad-ms", str(a.trim_pad_ms), "--trim-min-ms", str(a.trim_min_ms)]
    return out


def _reservoir_args(a):
    out = []
    for flag, v in (("--num-neurons", a.num_neurons), ("--num-output-neurons", a.num_output_neurons),
                    ("--small-world-k", a.small_world_k), ("--seed", a.seed)):
        if v is not None:
            out += [flag, str(v)]
    return out


STAGES = (
    ("Step 1: Creating Spike Train Dataset",
     lambda a: ["create_dataset.py", "--n-filters", str(a.n_filters), "--filterbank", a.filterbank]
     + _corpus_args(a) + (["--packed"] if a.packed else []) + _augment_args(a) + _reverb_args(a)
     + _speed_args(a) + _mask_args(a) + _variable_length_args(a)),
    ("Step 2: Extracting LSM Features",
     lambda a: ["extract_lsm_features.py", "--feature-set", a.feature_set, "--multiplier", str(a.multiplier)]
     + _reservoir_args(a) + (["--time-segments", str(a.time_segments)] if a.time_segments != 1 else [])
     + (["--model-out", a.save_model, "--filterbank", a.filterbank, "--n-filters", str(a.n_filters)] if a.save_model else [])),
    ("Step 3: Training and Evaluating Classifier",
     lambda a: ["train_classifier.py"] + (["--readout", a.readout] if a.readout else [])
     + (["--commands", a.commands] if a.commands else [])
     + (["--commands-file", a.commands_file] if a.commands_file else [])
     + (["--model-out", a.save_model] if a.save_model else [])),
)

IN_MEMORY = """import argparse, sys, create_dataset as cd, extract_lsm_features as ex
a = argparse.Namespace(**{ns!r})
augment = cd.augment_from_args(a)
audio, labels = cd.collect_audio(commands=cd.commands_from_args(a), dataset_root=a.dataset_root,
                                 max_per_class=cd.MAX_SAMPLES_PER_CLASS if a.max_per_class is None else a.max_per_class,
                                 synthetic_per_class=a.synthetic_per_class)
corrupt = cd.corruption(augment, len(audio)) if augment else None
room = cd.reverb_from_args(a)
reverb = cd.reverberation(room, len(audio)) if room else None
pace = cd.speed_from_args(a)
speed = cd.speeds(pace, len(audio)) if pace else None
ex.main_from_audio(audio, labels, a.n_filters, a.filterbank, a.feature_set, a.multiplier,
                   num_neurons=a.num_neurons, num_output_neurons=a.num_output_neurons,
                   small_world_k=a.small_world_k, seed=a.seed, readout=a.device_readout,
                   class_names=cd.commands_from_args(a), time_segments=a.time_segments, corrupt=corrupt, reverb=reverb,
                   speed=speed, **({{}} if cd.mask_from_args(a) is None else {{"mask": cd.mask_from_args(a)}}),
                   **({{"model_out": a.save_model}} if a.save_model else {{}}))
"""
# --readout stream-ridge: the same call with the passes over the training split, the penalty and the plans of the later passes
_LAST = """                   **({{"model_out": a.save_model}} if a.save_model else {{}}))
"""
IN_MEMORY_STREAM_RIDGE = IN_MEMORY[:-len(_LAST)] + """                   **({{"model_out": a.save_model}} if a.save_model else {{}}),
                   epochs=a.augment_epochs, ridge_alpha=a.ridge_alpha,
                   epoch_plans=lambda e: cd.epoch_plans(e, len(audio), augment, corrupt, room, reverb, pace))
"""
assert IN_MEMORY.endswith(_LAST)


def _launch(script_args, nproc: int):
    """One process, or `nproc` ranks of it (one per GPU) through torch.distributed.run."""
    if nproc <= 1:
        return [sys.executable] + script_args
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # inherited by the ranks: dmabuf IPC, which RCCL needs here
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
            "--master-addr", "127.0.0.1", "--master-port", os.environ.get("LSM_MASTER_PORT", "29517")] + script_args


def run_pipeline(n_filters: int, filterbank: str, feature_set: str, multiplier: float, in_memory: bool = False,
                 **extra):
    """1. spike-train dataset, 2. LSM features, 3. readout.  A failing stage does not stop the
    next one (the reference discards exit codes too); it shows up as that stage's own message.
    `in_memory` (not in the reference): stages 1 and 2 run as ONE process (or one per GPU) that keeps audio,
    rasters and features on the GPU (extract_lsm_features.main_from_audio; no File 1), then the readout as usual --
    except that a PyTorch readout (`readout="torch-ridge"` / `"torch-logistic"`) runs inside that process on the
    feature rows still on the GPU and prints the final report itself (no stage 3 process, no File 2 reload).
    `extra`: the forwarded constants (commands, commands_file, dataset_root, max_per_class, synthetic_per_class,
    packed, num_neurons, num_output_neurons, small_world_k, seed, readout, nproc, time_segments, and the corruption flags
    noise_dir, snr_db, time_shift_ms, level_db, augment_seed, the reverberation flags rir_dir, rir_prob, rir_max_ms and the
    speed flags speed_factors, speed_prob and the mask flags freq_masks, freq_mask_width, time_masks, time_mask_width,
    mask_prob: applied to stage 1 and to the in-memory route; variable_length, max_seconds: stage 1 keeps every clip at its
    own length, SPEC.md 1.14, and stage 2 finds the lengths in File 1; trim_silence, trim_pad_ms, trim_min_ms: stage 1 first
    cuts every such clip to its speech on the GPU, SPEC.md 1.15; augment_variable_length: stage 1 lets the corruption, the
    reverberation and the mask flags through on such clips, SPEC.md 1.16; speed_variable_length: beside it, stage 1 lets the
    speed flags through on such clips, SPEC.md 1.18; save_model: a path -- stage 2 writes the front half
    of the model file there and stage 3 adds its readout, or the in-memory route with a PyTorch readout writes it whole,
    SPEC.md 6; classify.py labels new audio with it; readout="stream-ridge" with augment_epochs, ridge_alpha: the in-memory
    route trains a ridge readout from statistics updated on the GPU, SPEC.md 7, and keeps no training row)."""
    args = argparse.Namespace(n_filters=n_filters, filterbank=filterbank, feature_set=feature_set,
                              multiplier=multiplier, commands=None, commands_file=None, dataset_root=None,
                              max_per_class=None, synthetic_per_class=int(os.environ.get("LSM_SYNTHETIC_PER_CLASS", "0")),
                              packed=False, num_neurons=None, num_output_neurons=None, small_world_k=None, seed=None,
                              readout=None, nproc=1, time_segments=1, noise_dir=None, snr_db=None, time_shift_ms=0.0,
                              level_db=None, augment_seed=42, rir_dir=None, rir_prob=1.0, rir_max_ms=500.0,
                              speed_factors=None, speed_prob=1.0, freq_masks=0, freq_mask_width=0, time_masks=0,
                              time_mask_width=0, mask_prob=1.0, variable_length=False, max_seconds=1.0,
                              trim_silence=None, trim_pad_ms=30.0, trim_min_ms=30.0, augment_variable_length=False,
                              speed_variable_length=False, save_model=None, augment_epochs=None, ridge_alpha=None)
    unknown = set(extra) - set(vars(args))
    if unknown:
        raise TypeError(f"run_pipeline: unknown arguments {sorted(unknown)}")
    vars(args).update(extra)
    streamed = args.readout == "stream-ridge"
    if streamed and not in_memory:
        raise SystemExit("--readout stream-ridge needs --in-memory: the statistics are updated as the feature rows leave the "
                         "reservoir, and the file route keeps every row in File 2")
    if not streamed and (args.augment_epochs is not None or args.ridge_alpha is not None):
        raise SystemExit("--augment-epochs and --ridge-alpha need --readout stream-ridge: the other readouts keep every "
                         "training row once and fix their own penalty")
    if streamed:
        args.augment_epochs = 1 if args.augment_epochs is None else int(args.augment_epochs)
        args.ridge_alpha = 1.0 if args.ridge_alpha is None else float(args.ridge_alpha)
        if args.augment_epochs < 1:
            raise SystemExit(f"--augment-epochs {args.augment_epochs}: must be >= 1")
        if args.time_segments != 1:
            raise SystemExit("--readout stream-ridge needs --time-segments 1: the statistics hold one feature row per clip")
    else:
        del args.augment_epochs, args.ridge_alpha          # without the new flags every command is what it was
    if args.trim_silence is not None and not args.variable_length:
        raise SystemExit("--trim-silence needs --variable-length: a trimmed clip has a length of its own")
    if args.variable_length and (in_memory or args.nproc > 1):
        raise SystemExit("--variable-length goes through File 1 in one process: it combines with neither --in-memory nor --nproc")
    print("--- Running Pipeline ---")
    if in_memory:
        print("\n--- Steps 1+2: audio -> LSM features on the GPU (no dataset file) ---", flush=True)
        ns = {k: v for k, v in vars(args).items() if k not in ("readout", "nproc", "packed", "speed_variable_length")}
        # a PyTorch readout on the in-memory route runs where the features already are: scaler, readout and
        # predictions on the GPU, no File 2 reload; File 2 is still written
        device_readout = args.readout if args.readout in ("torch-ridge", "torch-logistic", "stream-ridge") else None
        ns["device_readout"] = device_readout
        code = f"import sys; sys.path.insert(0, {HERE!r})\n" + (IN_MEMORY_STREAM_RIDGE if streamed else IN_MEMORY).format(ns=ns)
        if args.nproc > 1:            # torch.distributed.run needs a file to start
            import tempfile
            with tempfile.NamedTemporaryFile("w", suffix="_lsm_in_memory.py", delete=False) as fh:
                fh.write(code)
            try:
                subprocess.call(_launch([fh.name], args.nproc))
            finally:
                os.unlink(fh.name)
        else:
            subprocess.call([sys.executable, "-c", code])
        stages = () if device_readout else STAGES[2:]
    else:
        stages = STAGES
    for i, (title, command) in enumerate(stages):
        print(f"\n--- {title} ---", flush=True)
        cmd = command(args)
        sharded = not in_memory and i < 2
        subprocess.call(_launch([os.path.join(HERE, cmd[0])] + cmd[1:], args.nproc if sharded else 1))
    print("\n--- Pipeline Finished ---")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Run the entire speech recognition pipeline.")
    ap.add_argument("--n-filters", type=int, default=128, help="Number of filters for the filterbank.")
    ap.add_argument("--filterbank", type=str, default="gammatone", choices=["mel", "gammatone"],
                    help="Type of filterbank to use.")
    ap.add_argument("--feature-set", type=str, default="original",
                    choices=['all', 'rate', 'timing', 'rhythm', 'original'],
                    help="The set of features to extract.")
    ap.add_argument("--multiplier", type=float, default=0.6, help="Multiplier for w_critico.")
    ap.add_argument("--in-memory", action="store_true", default=os.environ.get("LSM_IN_MEMORY", "0") == "1",
                    help="Run stages 1 and 2 in one process on the GPU without writing the dataset file.")
    # --- the reference's hard-coded constants, forwarded to the stages (defaults: the reference's values) ---
    ap.add_argument("--commands", type=str, default=None, help="Comma-separated class list (stage 1, report names).")
    ap.add_argument("--commands-file", type=str, default=None, help="File with one class name per line.")
    ap.add_argument("--dataset-root", type=str, default=None, help="Corpus folder (stage 1).")
    ap.add_argument("--max-per-class", type=int, default=None, help="Per-class cap on the sorted file list (stage 1).")
    ap.add_argument("--synthetic-per-class", type=int, default=int(os.environ.get("LSM_SYNTHETIC_PER_CLASS", "0")),
                    help="Synthetic clips per class instead of wav files (stage 1).")
    ap.add_argument("--packed", action="store_true", help="Bit-packed File 1 (stage 1).")
    ap.add_argument("--num-neurons", type=int, default=None, help="Reservoir size (stage 2; default 1000).")
    ap.add_argument("--num-output-neurons", type=int, default=None, help="Read-out neurons (stage 2; default 400).")
    ap.add_argument("--small-world-k", type=int, default=None, help="Ring neighbours (stage 2; default int(0.2 N)).")
    ap.add_argument("--seed", type=int, default=None, help="Reservoir wiring seed (stage 2; default 42).")
    ap.add_argument("--readout", type=str, default=None, choices=["sklearn", "torch-ridge", "torch-logistic", "stream-ridge"],
                    help="Readout of stage 3 (default: scikit-learn logistic regression, or LSM_READOUT).  stream-ridge "
                         "(with --in-memory): a ridge readout trained from statistics updated on the GPU, no training row kept.")
    ap.add_argument("--augment-epochs", type=int, default=None, metavar="E",
                    help="With --readout stream-ridge: run the training split E times, epoch e with the augmentation plans "
                         "of --augment-seed + e (default 1).")
    ap.add_argument("--ridge-alpha", type=float, default=None, metavar="A",
                    help="With --readout stream-ridge: the ridge penalty (default 1.0).")
    ap.add_argument("--nproc", type=int, default=int(os.environ.get("LSM_NPROC", "1")),
                    help="Ranks (one per GPU) for stages 1 and 2.")
    ap.add_argument("--time-segments", type=int, default=1,
                    help="Read every clip in K equal time segments, K feature rows side by side (stage 2; default 1).")
    ap.add_argument("--noise-dir", type=str, default=None,
                    help="Folder of background-noise wav files mixed into every clip on the GPU, or 'synthetic' (stage 1).")
    ap.add_argument("--snr-db", type=str, default=None, help="SNR in dB, A or a range A,B drawn per clip (stage 1).")
    ap.add_argument("--time-shift-ms", type=float, default=0.0, help="Random time shift of up to this many ms (stage 1).")
    ap.add_argument("--level-db", type=str, default=None, help="Level change in dB, A or a range A,B (stage 1).")
    ap.add_argument("--augment-seed", type=int, default=42, help="Seed of the per-clip corruption draws (stage 1).")
    ap.add_argument("--rir-dir", type=str, default=None,
                    help="Folder of room-impulse-response wav files convolved with every clip on the GPU, or 'synthetic' "
                         "(stage 1).")
    ap.add_argument("--rir-prob", type=float, default=1.0, help="Share of the clips that are reverberated (stage 1).")
    ap.add_argument("--rir-max-ms", type=float, default=500.0, help="Cut every response to this many ms (stage 1).")
    ap.add_argument("--speed-factors", type=str, default=None,
                    help="Comma-separated playback speeds drawn per clip on the GPU, e.g. 0.9,1.0,1.1 (stage 1).")
    ap.add_argument("--speed-prob", type=float, default=1.0, help="Share of the clips whose speed is drawn (stage 1).")
    ap.add_argument("--freq-masks", type=int, default=0, help="Frequency bands zeroed per clip inside the encoder (stage 1).")
    ap.add_argument("--freq-mask-width", type=int, default=0, help="Largest width of a frequency band, in filters (stage 1).")
    ap.add_argument("--time-masks", type=int, default=0, help="Time spans zeroed per clip inside the encoder (stage 1).")
    ap.add_argument("--time-mask-width", type=int, default=0, help="Largest width of a time span, in time bins (stage 1).")
    ap.add_argument("--mask-prob", type=float, default=1.0, help="Share of the clips that are masked (stage 1).")
    ap.add_argument("--variable-length", action="store_true",
                    help="Keep every clip at its own length instead of padding it to one second (stage 1; stage 2 reads the "
                         "lengths from File 1).")
    ap.add_argument("--max-seconds", type=float, default=1.0, help="With --variable-length: trim clips at this length (stage 1).")
    ap.add_argument("--trim-silence", type=float, default=None, metavar="DB",
                    help="With --variable-length: cut every clip on the GPU to the bins within DB decibels of its loudest (stage 1).")
    ap.add_argument("--trim-pad-ms", type=float, default=30.0, help="With --trim-silence: kept around the speech (stage 1).")
    ap.add_argument("--trim-min-ms", type=float, default=30.0, help="With --trim-silence: shortest trimmed clip (stage 1).")
    ap.add_argument("--augment-variable-length", action="store_true",
                    help="With --variable-length: let the corruption flags, --rir-dir and the mask flags through (stage 1).")
    ap.add_argument("--speed-variable-length", action="store_true",
                    help="With --variable-length --augment-variable-length: let the speed flags through (stage 1).")
    ap.add_argument("--save-model", type=str, default=None, metavar="PATH",
                    help="Save the trained model (scaler, readout, front-end and reservoir parameters) for classify.py "
                         "(stages 2 and 3).")
    a = ap.parse_args()
    run_pipeline(n_filters=a.n_filters, filterbank=a.filterbank, feature_set=a.feature_set,
                 multiplier=a.multiplier, in_memory=a.in_memory, commands=a.commands, commands_file=a.commands_file,
                 dataset_root=a.dataset_root, max_per_class=a.max_per_class,
                 synthetic_per_class=a.synthetic_per_class, packed=a.packed, num_neurons=a.num_neurons,
                 num_output_neurons=a.num_output_neurons, small_world_k=a.small_world_k, seed=a.seed,
                 readout=a.readout, nproc=a.nproc, time_segments=a.time_segments, noise_dir=a.noise_dir, snr_db=a.snr_db,
                 time_shift_ms=a.time_shift_ms, level_db=a.level_db, augment_seed=a.augment_seed,
                 rir_dir=a.rir_dir, rir_prob=a.rir_prob, rir_max_ms=a.rir_max_ms, speed_factors=a.speed_factors,
                 speed_prob=a.speed_prob, freq_masks=a.freq_masks, freq_mask_width=a.freq_mask_width,
                 time_masks=a.time_masks, time_mask_width=a.time_mask_width, mask_prob=a.mask_prob,
                 variable_length=a.variable_length, max_seconds=a.max_seconds, trim_silence=a.trim_silence,
                 trim_pad_ms=a.trim_pad_ms, trim_min_ms=a.trim_min_ms, augment_variable_length=a.augment_variable_length,
                 speed_variable_length=a.speed_variable_length, save_model=a.save_model, augment_epochs=a.augment_epochs, ridge_alpha=a.ridge_alpha)
