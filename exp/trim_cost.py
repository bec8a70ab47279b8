"""Writes profiles/silence_trim.txt (`--out`; printed as well).  Four parts.

The code object: csrc/trim.hip compiled with the build's flags and `-Rpass-analysis=kernel-resource-usage`, the compiler's
own report of `trim_kernel` -- registers, scratch, spills, occupancy, static LDS -- beside the dynamic LDS of a launch
(`lsm_trim_lds_bytes`).  Needs hipcc, no GPU (`--no-timing` stops here).

The trim launch: 256 quiet synthetic clips of 16000 samples (`class_chirps(noise=0.001)`), `lsm_trim_silence_f32` at 30 dB
with 3 bins of padding, beside three figures of the same process, the forms alternating: a device-to-device copy of the
same 16.4 MB (the floor of anything that reads and writes the batch once), the launch on counts of 0 (no energies, nothing
copied: the zero fill of the rows alone), and the ragged gammatone front-end launch on the trimmed clips that the trim
feeds (128 filters, longest first) with the same launch on the untrimmed clips.  Device events, medians of 20 after 4
warm-up launches, `--rounds` times over.

The payoff: `pipeline.features_from_utterances` on the 256 clips at cfg2's reservoir (1000 neurons, k = 200, 400 output
neurons, w_critico * 0.6), untrimmed against `trim=SilenceTrimmer(30, 3, 3)`, unfused and `fused=True`; a host clock around
the call and a device synchronise, the four forms alternating, medians of 5 after a warm-up call each.

Accuracy: the synthetic 12 classes (40 clips per class at noise 0.001, an 80 / 20 split, the ridge readout on the device),
untrimmed against trimmed.  One run per cell, untuned; nothing is asserted."""
import argparse
import collections
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-timing", action="store_true", help="the code object only (no GPU needed)")
ap.add_argument("--no-accuracy", action="store_true")
args = ap.parse_args()

lines = []


def code_object():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc] + build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
                                                     "-c", os.path.join(build.PKG_DIR, "csrc", "trim.hip"), "-o",
                                                     os.path.join(tmp, "trim.o")], capture_output=True, text=True, check=True)
    report = [m.group(1).strip() for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr)]
    lines.append("trim_kernel, the compiler's resource report (hipcc " + " ".join(build.CFLAGS) + "):")
    lines.extend("  " + ln for ln in report)
    fields = dict(ln.split(": ", 1) for ln in report if ": " in ln)
    assert fields["ScratchSize [bytes/lane]"] == "0" and fields["VGPRs Spill"] == "0", "trim_kernel uses scratch"


code_object()

if not args.no_timing:
    import torch
    import trim_restatement as TR
    from lsm_speech_classifier_amd import _lib, frontend, pipeline, reservoir, snn, synth
    from oracle import ref_numpy

    lib = _lib.load()
    _lib.require_gpu()
    B, N, TB, HOP, F = 256, 16000, 100, 160, 128
    lds = lib.lsm_trim_lds_bytes(TB)
    lines += [f"  dynamic LDS of a launch: {lds} bytes at time_bins = {TB} ({160 * 1024 // (lds + 24)} workgroups of 4 waves per "
              f"CU by LDS), {lib.lsm_trim_lds_bytes(4096)} at 4096",
              f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}",
              f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}"]
    labels = np.arange(B) % 12
    quiet_h = synth.class_chirps(labels, seed=1234, noise=0.001)
    quiet = torch.from_numpy(quiet_h).cuda()
    trimmer = frontend.SilenceTrimmer(30.0, 3, 3)
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    out = torch.empty_like(quiet)
    first, bins = (torch.empty((B,), dtype=torch.int32, device="cuda") for _ in range(2))
    zeros = torch.zeros((B,), dtype=torch.int32, device="cuda")

    def trim_launch(counts):
        def go():
            assert lib.lsm_trim_silence_f32(void(quiet), B, N, TB, void(counts), C.c_double(trimmer.ratio), 3, 3, void(out), N,
                                            void(first), void(bins), None, stream) == 0
        return go

    trim_launch(None)()
    torch.cuda.synchronize()
    want = TR.trim(quiet_h, None, TB, trimmer.ratio, 3, 3)
    same = out.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(bins.cpu().numpy(), want[2])
    kept = want[2].astype(np.int64)
    lines.append(f"{B} clips x {N} samples, class_chirps(noise=0.001), top_db 30, pad 3, min 3: trimmed to {kept.min()} .. {kept.max()} "
                 f"bins, mean {kept.mean():.1f}, {int((kept == TB).sum())} kept whole; the launch equals the restatement byte for "
                 f"byte: {same}")
    loud = TR.trim(synth.class_chirps(labels[:48], seed=1234), None, TB, trimmer.ratio, 3, 3)[2]
    lines.append(f"  at the default noise = 0.04 (background about 10 dB under the peak bin) {int((loud == TB).sum())} of 48 clips are "
                 f"kept whole at 30 dB: nothing trims")

    fe = frontend.SpikeFrontEnd(F, "gammatone")
    order = np.argsort(-kept, kind="stable")
    trimmed_sorted = out[torch.from_numpy(order).cuda()].contiguous()
    bins_sorted = torch.from_numpy(kept[order].astype(np.int32)).cuda()
    full = torch.full((B,), TB, dtype=torch.int32, device="cuda")
    raster = torch.empty((B, fe.n_channels, fe.n_steps), dtype=torch.uint8, device="cuda")
    ws = fe.new_workspace(B)
    copy_dst = torch.empty_like(quiet)
    forms = [("lsm_trim_silence_f32                         ", trim_launch(None)),
             ("device-to-device copy of the 16.4 MB         ", lambda: copy_dst.copy_(quiet)),
             ("trim launch, all counts 0 (zero fill alone)  ", trim_launch(zeros)),
             ("ragged front end, trimmed clips longest first", lambda: fe.encode_ragged(trimmed_sorted, bins_sorted, fused=True,
                                                                                       raster_out=raster, workspace=ws)),
             ("ragged front end, untrimmed clips (100 bins) ", lambda: fe.encode_ragged(quiet, full, fused=True, raster_out=raster,
                                                                                       workspace=ws))]

    def timed(fn, reps=20, warm=4):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    med = collections.defaultdict(list)
    for rnd in range(1, args.rounds + 1):
        for name, fn in forms:
            t = timed(fn)
            med[name].append(t[0])
            lines.append(f"  round {rnd}: {name}  median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
    m = {name: float(np.median(v)) for name, v in med.items()}
    for name, v in med.items():
        lines.append(f"  {name}: median of the rounds {m[name]:8.1f} us, rounds between {min(v):.1f} and {max(v):.1f}")
    t_trim, t_copy, t_fill, t_fe, t_fe_full = (m[name] for name, _ in forms)
    lines.append(f"  the trim launch is {t_trim / t_copy:.2f} x the copy and {t_trim / t_fe:.3f} of the front-end launch it feeds "
                 f"({t_trim / t_fe_full:.3f} of the untrimmed one; the front end's share of samples is {kept.sum() / (B * TB):.3f}, "
                 f"its time {t_fe / t_fe_full:.3f})")
    if t_trim > 0.1 * t_fe:
        lines.append(f"  more than a tenth of that launch: of the trim's {t_trim:.1f} us the zero fill alone takes {t_fill:.1f}; the rest, "
                     f"{t_trim - t_fill:.1f} us, is the energies (staging and the 160-step sum of one wave per 64 bins) and the copy's reads")

    # ---- payoff -----------------------------------------------------------------------------------------------------------
    k = 200
    head = fe.encode(quiet).cpu().numpy()
    wc = ref_numpy.w_critico(k, 2.0, 2, head)
    params = reservoir.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=k, mean_weight=wc * 0.6)
    net = snn.SNN(params, n_channels=fe.n_channels)
    utts = list(quiet_h)
    calls = [("untrimmed, two launches", dict()), ("trimmed,   two launches", dict(trim=trimmer)),
             ("untrimmed, fused=True  ", dict(fused=True)), ("trimmed,   fused=True  ", dict(trim=trimmer, fused=True))]
    lines.append(f"features_from_utterances, {B} clips, cfg2's reservoir (N 1000, k 200, 400 output neurons); ragged fused step "
                 f"served: {pipeline.step_fused_supported(fe, net, B, 'ragged')}")
    took = collections.defaultdict(list)
    for name, kw in calls:
        pipeline.features_from_utterances(utts, fe, net, None, **kw)
    torch.cuda.synchronize()
    for rep in range(5):
        for name, kw in calls:
            t0 = time.perf_counter()
            pipeline.features_from_utterances(utts, fe, net, None, **kw)
            torch.cuda.synchronize()
            took[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in took.items():
        lines.append(f"  {name}: median of 5 {np.median(v):8.2f} ms (min {min(v):.2f}, max {max(v):.2f})")
    for a, b in ((calls[1][0], calls[0][0]), (calls[3][0], calls[2][0])):
        lines.append(f"  {a.strip()} / {b.strip()} = {np.median(took[a]) / np.median(took[b]):.3f}")
    # the device work alone: the batches' launches on rows already on the device
    bins_h = kept[order].astype(np.int32)
    steps_full = np.full(B, TB, dtype=np.int32)

    def device_only(x, b):
        def go():
            r, s = fe.encode_ragged(x, b, raster_out=raster, workspace=ws)
            net.run_batch(r, None, lengths=s)
        return go
    dev = {}
    for name, fn in (("untrimmed", device_only(quiet, steps_full)), ("trimmed, longest first", device_only(trimmed_sorted, bins_h))):
        dev[name] = timed(fn, reps=9, warm=3)
        lines.append(f"  device work of one batch, front end + reservoir, {name}: median {dev[name][0]:8.1f} us "
                     f"(min {dev[name][1]:.1f}, max {dev[name][2]:.1f})")
    lines.append(f"  trimmed / untrimmed device work = {dev['trimmed, longest first'][0] / dev['untrimmed'][0]:.3f}; longest clip "
                 f"{kept.max() / TB:.2f} of the full length, samples {kept.sum() / (B * TB):.3f}")

    # ---- accuracy ---------------------------------------------------------------------------------------------------------
    if not args.no_accuracy:
        from sklearn.model_selection import train_test_split
        from lsm_speech_classifier_amd import readout as ro
        y_all = np.repeat(np.arange(12), 40).astype(np.int32)
        clips = list(synth.class_chirps(y_all, seed=1234, noise=0.001))
        i_tr, i_te, y_tr, y_te = train_test_split(np.arange(len(clips)), y_all, test_size=0.2, random_state=42, stratify=y_all)
        lines.append("accuracy, synthetic 12 classes x 40 clips (noise 0.001), 80 / 20 split, ridge readout, one run, untuned:")
        for name, kw in (("untrimmed", dict()), ("trimmed 30 dB", dict(trim=trimmer))):
            X = pipeline.features_from_utterances(clips, fe, net, None, **kw)
            scaler = ro.StandardScaler()
            model = ro.RidgeReadout(1.0).fit(scaler.fit_transform(X[torch.from_numpy(i_tr).cuda()]),
                                             torch.from_numpy(y_tr).to(fe.device))
            acc = float((model.predict(scaler.transform(X[torch.from_numpy(i_te).cuda()])).cpu().numpy() == y_te).mean())
            lines.append(f"  {name:14s} test accuracy {100 * acc:6.2f} %")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
