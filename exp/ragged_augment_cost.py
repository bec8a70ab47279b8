"""Writes profiles/ragged_augment.txt (`--out`; printed as well).  Two parts, which may run apart (`--no-timing`, `--no-code`).

The code objects (needs hipcc, no GPU): csrc/mix.hip, csrc/ragged_masked_frontend.hip and csrc/step_fused_ragged_masked.hip
compiled with the build's flags and `-Rpass-analysis=kernel-resource-usage` -- VGPRs, SGPRs, scratch, static LDS and occupancy
of every new kernel from the compiler's own report; none may use scratch.  With `--parent-csrc DIR` (the csrc/ of the parent
commit, its include/ beside it) the units that existed there are compiled from both trees and their reports compared kernel by
kernel: the existing kernels must keep theirs.

The launches (an MI355X, device events, forms alternating, medians of 20 after 4 warm-up launches, `--rounds` times over):
  (a) `lsm_mix_ragged_f32` at 256 x 16000 with all lengths full, beside `lsm_mix_f32` of this build and, with `--parent-lib`,
      of the parent build's library (loaded beside this one);
  (b) the same launch with lengths uniform in 0.3 .. 1.0 s;
  (c) `lsm_gammatone_spikes_ragged_masked_f64` beside `lsm_gammatone_spikes_ragged_f64` (this build's, and the parent's with
      `--parent-lib`) at 256 x 128 filters, at full length and at those lengths, longest first;
  (d) the masked ragged one-launch step beside the ragged step at cfg2's reservoir (the ragged step's code object is the
      parent's: see the first part);
  (e) `pipeline.features_from_utterances` end to end with and without the chain (trim, reverberation, mixer, masks), a host
      clock around the call and a device synchronise, medians of 5.
Then the accuracy on the synthetic 12 classes with the chain on trimmed clips, trained and tested with and without it: one
run per cell, untuned.  Nothing is asserted
beyond "no scratch" and "the existing reports are unchanged"."""
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
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-timing", action="store_true", help="the code objects only (no GPU needed)")
ap.add_argument("--no-code", action="store_true", help="the launches only")
ap.add_argument("--no-accuracy", action="store_true")
ap.add_argument("--parent-csrc", default=None, help="csrc/ of the parent commit: compare the existing kernels' reports")
ap.add_argument("--parent-lib", default=None, help="liblsm_hip.so of the parent commit: time its entry points beside this build's")
args = ap.parse_args()

lines = []
NEW_UNITS = ["mix.hip", "ragged_masked_frontend.hip", "step_fused_ragged_masked.hip"]
OLD_UNITS = ["mix.hip", "frontend.hip", "mask.hip", "ragged_frontend.hip", "mel.hip", "step_fused.hip", "step_fused_masked.hip",
             "step_fused_ragged.hip", "step_fused_state.hip"]
FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("LDS", "LDS Size [bytes/block]"), ("waves/SIMD", "Occupancy [waves/SIMD]")]


def reports(csrc, include, unit):
    """{kernel name (demangled, without its arguments): {field: value}} of one translation unit."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc] + build.CFLAGS + ["-I", include, "-Rpass-analysis=kernel-resource-usage", "-c",
                                                     os.path.join(csrc, unit), "-o", os.path.join(tmp, "unit.o")],
                           capture_output=True, text=True, check=True)
    out, cur = collections.OrderedDict(), None
    for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr):
        text = m.group(1).strip()
        if text.startswith("Function Name: "):
            name = subprocess.run(["c++filt", text.split(": ", 1)[1]], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", name))
            cur = out.setdefault(re.sub(r"\(.*$", "", name), {})
        elif cur is not None and ": " in text:
            k, v = text.split(": ", 1)
            cur[k] = v
    return out


def code_objects():
    csrc, include = os.path.join(build.PKG_DIR, "csrc"), os.path.join(ROOT, "include")
    units = sorted(set(NEW_UNITS) | (set(OLD_UNITS) if args.parent_csrc else set()))
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS") or 16)) as ex:
        mine = dict(zip(units, ex.map(lambda u: reports(csrc, include, u), units)))
        theirs = {}
        if args.parent_csrc:
            p_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(args.parent_csrc))), "include")
            theirs = dict(zip(OLD_UNITS, ex.map(lambda u: reports(args.parent_csrc, p_inc, u), OLD_UNITS)))
    lines.append("the new kernels, the compiler's resource report (hipcc " + " ".join(build.CFLAGS) + "):")
    lines.append(f"  {'kernel':68s} " + " ".join(f"{h:>10s}" for h, _ in FIELDS))
    for unit in NEW_UNITS:
        for name, f in mine[unit].items():
            if unit == "mix.hip" and name != "mix_kernel<true>":
                continue
            lines.append(f"  {name:68s} " + " ".join(f"{f.get(k, '-'):>10s}" for _, k in FIELDS))
            assert f["ScratchSize [bytes/lane]"] == "0" and f.get("VGPRs Spill", "0") == "0", f"{name} uses scratch"
    lines.append("  no new kernel uses scratch or spills a register")
    if args.parent_csrc:
        rename = {"mix_kernel": "mix_kernel<false>"}                # the batch kernel became the RAGGED = false form of a template
        total = changed = 0
        for unit in OLD_UNITS:
            for name, f in theirs[unit].items():
                total += 1
                now = mine[unit].get(rename.get(name, name))
                if now != f:
                    changed += 1
                    lines.append(f"  CHANGED {unit} {name}: {f} -> {now}")
        lines.append(f"the existing kernels against the parent's sources: {total} kernels of {len(OLD_UNITS)} units "
                     f"({', '.join(OLD_UNITS)}), {changed} with another report")
        assert changed == 0, "an existing kernel's resource report changed"


if not args.no_code:
    code_objects()

if not args.no_timing:
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, pipeline, reservoir, snn, synth
    from oracle import ref_numpy

    lib = _lib.load()
    _lib.require_gpu()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        for table in (_lib._SIGS, _lib.MIX_SIGS, _lib.RAGGED_SIGS):
            for name, (res, argtypes) in table.items():
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, argtypes
        lines.append(f"parent library: build id {parent.lsm_build_id().decode()}")
    B, N, TB, HOP, F = 256, 16000, 100, 160, 128
    lines += [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}",
              f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}"]
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    host = lambda a: C.c_void_p(a.ctypes.data)                                  # noqa: E731
    labels = np.arange(B) % 12
    quiet_h = synth.class_chirps(labels, seed=1234, noise=0.001)
    audio = torch.from_numpy(quiet_h).cuda()
    rs = np.random.RandomState(7)
    bins_h = np.sort(rs.randint(30, TB + 1, size=B))[::-1].astype(np.int32).copy()      # 0.3 .. 1.0 s, longest first
    full_bins = torch.full((B,), TB, dtype=torch.int32, device="cuda")
    some_bins = torch.from_numpy(bins_h).cuda()
    lines.append(f"{B} clips x {N} samples; ragged lengths uniform in 30 .. {TB} bins, longest first: mean {bins_h.mean():.1f} bins")

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

    def compare(title, forms):
        lines.append(title)
        med = collections.defaultdict(list)
        for rnd in range(1, args.rounds + 1):
            for name, fn in forms:
                t = timed(fn)
                med[name].append(t[0])
                lines.append(f"  round {rnd}: {name}  median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
        for name, v in med.items():
            lines.append(f"  {name}: median of the rounds {np.median(v):8.1f} us, rounds between {min(v):.1f} and {max(v):.1f}")
        return {name: (float(np.median(v)), min(v), max(v)) for name, v in med.items()}

    def beside(m, a, b):
        (ta, lo_a, hi_a), (tb, lo_b, hi_b) = m[a], m[b]
        inside = lo_a <= hi_b and lo_b <= hi_a
        lines.append(f"  {a.strip()} / {b.strip()} = {ta / tb:.3f} ({100 * (ta / tb - 1):+.1f} %); the rounds' ranges "
                     f"{'overlap: inside the run-to-run spread' if inside else 'are APART: outside the run-to-run spread'}")

    # ---- (a), (b): the mixer ----------------------------------------------------------------------------------------------
    noise = torch.from_numpy(synth.white_noise(4, seed=3, n_samples=N) * np.float32(0.1)).cuda()
    plan = frontend.mix_plan(B, 4, N, (5.0, 15.0), max_shift=1600, seed=4)
    per_clip = [torch.from_numpy(a).cuda() for a in (plan.rows, plan.offsets, plan.shift, plan.scale,
                                                     frontend.snr_ratio(plan.snr_db, B))]
    mixed = torch.empty_like(audio)
    full_samples, some_samples = full_bins * HOP, some_bins * HOP

    def mix(which, lengths=None):
        head = [void(audio), B, N] + ([void(lengths)] if lengths is not None else [])
        fn = getattr(which, "lsm_mix_f32" if lengths is None else "lsm_mix_ragged_f32")

        def go():
            assert fn(*head, void(noise), 4, N, *[void(t) for t in per_clip], void(mixed), None, None, stream) == 0
        return go

    forms = [("(a) lsm_mix_ragged_f32, all lengths full    ", mix(lib, full_samples)),
             ("    lsm_mix_f32, this build                 ", mix(lib))]
    if parent is not None:
        forms.append(("    lsm_mix_f32, parent build               ", mix(parent)))
    forms.append(("(b) lsm_mix_ragged_f32, lengths 0.3 .. 1.0 s", mix(lib, some_samples)))
    m = compare("the mixer, 256 x 16000 samples, SNR 5 .. 15 dB, shifts up to 0.1 s:", forms)
    beside(m, forms[0][0], forms[2][0] if parent is not None else forms[1][0])
    beside(m, forms[-1][0], forms[0][0])

    # ---- (c): the front end -----------------------------------------------------------------------------------------------
    fe = frontend.SpikeFrontEnd(F, "gammatone")
    on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
    raster = torch.empty((B, fe.n_channels, fe.n_steps), dtype=torch.uint8, device="cuda")
    ws = fe.new_workspace(B)
    masks = {"full": frontend.mask_plan_ragged(np.full(B, TB), F, TB, 2, 15, 2, 20, seed=5),
             "some": frontend.mask_plan_ragged(bins_h, F, TB, 2, 15, 2, 20, seed=5)}
    words = {k: frontend.upload_mask(p, B, F, TB, fe.device) for k, p in masks.items()}
    layout = lib.lsm_gammatone_spikes_layout(B, F, 0)
    lines.append(f"front end: {F} filters, layout {layout} ({ {0: 'lane pair', 1: 'one chain', 2: 'two chains'}[layout]}); masks: 2 "
                 f"frequency bands of up to 15 filters, 2 time spans of up to 20 bins (SpecAugment's shape at this size)")

    def front(which, bins, mask=None):
        fn = getattr(which, "lsm_gammatone_spikes_ragged_f64" if mask is None else "lsm_gammatone_spikes_ragged_masked_f64")
        tail = [] if mask is None else [void(mask[0]), void(mask[1])]

        def go():
            assert fn(void(audio), B, N, void(fe.coefs), F, fe.nwin, fe.hop, fe.ncols, TB, void(bins), host(on), host(off), len(on),
                      fe.redundancy, void(raster), None, void(ws), ws.numel() * 8, fe.coef_flags, 0, *tail, stream) == 0
        return go

    forms = [("(c) ragged masked front end, full length    ", front(lib, full_bins, words["full"])),
             ("    ragged front end, full, this build      ", front(lib, full_bins))]
    if parent is not None:
        forms.append(("    ragged front end, full, parent build    ", front(parent, full_bins)))
    forms += [("    ragged masked front end, 0.3 .. 1.0 s   ", front(lib, some_bins, words["some"])),
              ("    ragged front end, 0.3 .. 1.0 s          ", front(lib, some_bins))]
    m = compare("the one-launch gammatone front end (the unragged mask costs +3.9 %: profiles/spec_mask.txt):", forms)
    beside(m, forms[0][0], forms[2][0] if parent is not None else forms[1][0])
    beside(m, forms[-2][0], forms[-1][0])

    # ---- (d): the fused step ----------------------------------------------------------------------------------------------
    k = 200
    wc = ref_numpy.w_critico(k, 2.0, 2, fe.encode(audio).cpu().numpy())
    net = snn.SNN(reservoir.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=k, mean_weight=wc * 0.6),
                  n_channels=fe.n_channels)
    served = pipeline.step_fused_supported(fe, net, B, "ragged-masked")
    lines.append(f"cfg2's reservoir (N 1000, k 200, 400 output neurons); masked ragged fused step served: {served}")
    if served:
        rows = torch.empty((B, 8 * net.num_output_neurons), dtype=torch.float32, device="cuda")

        def step(bins, mask=None):
            return lambda: pipeline.step_fused_ragged(fe, net, audio, bins, features_out=rows, workspace=ws,
                                                      **({} if mask is None else {"mask": mask}))
        forms = [("(d) masked ragged step, full length         ", step(full_bins, masks["full"])),
                 ("    ragged step, full length                ", step(full_bins)),
                 ("    masked ragged step, 0.3 .. 1.0 s        ", step(some_bins, masks["some"])),
                 ("    ragged step, 0.3 .. 1.0 s               ", step(some_bins))]
        m = compare("the one-launch step (through pipeline.step_fused_ragged: the masked form also uploads its words):", forms)
        beside(m, forms[0][0], forms[1][0])
        beside(m, forms[2][0], forms[3][0])

    # ---- (e): end to end --------------------------------------------------------------------------------------------------
    utts = [np.ascontiguousarray(c[:HOP * t]) for c, t in zip(quiet_h, bins_h)]
    trimmer = frontend.SilenceTrimmer(30.0, 3, 3)
    rir, rir_lengths = synth.room_responses(4, seed=5)
    rv = frontend.Reverberator(rir, rir_lengths)
    mixer = frontend.NoiseMixer(noise)
    chain = dict(trim=trimmer, reverb=(rv, frontend.reverb_plan(B, rv.n_rows, prob=0.5, seed=4)), corrupt=(mixer, plan),
                 mask=lambda bins: frontend.mask_plan_ragged(bins, F, TB, 2, 15, 2, 20, seed=5))
    calls = [("(e) no chain, two launches       ", dict()), ("    trim only, two launches      ", dict(trim=trimmer)),
             ("    whole chain, two launches    ", dict(chain)), ("    whole chain, fused=True      ", dict(chain, fused=True))]
    lines.append(f"features_from_utterances, {B} utterances of 0.3 .. 1.0 s, cfg2's reservoir:")
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
    lines.append(f"  whole chain / trim only = {np.median(took[calls[2][0]]) / np.median(took[calls[1][0]]):.3f}, whole chain / no chain = "
                 f"{np.median(took[calls[2][0]]) / np.median(took[calls[0][0]]):.3f}")

    # ---- accuracy ---------------------------------------------------------------------------------------------------------
    if not args.no_accuracy:
        from sklearn.model_selection import train_test_split
        from lsm_speech_classifier_amd import readout as ro
        y_all = np.repeat(np.arange(12), 40).astype(np.int32)
        clips = list(synth.class_chirps(y_all, seed=1234, noise=0.001))
        n = len(clips)
        i_tr, i_te, y_tr, y_te = train_test_split(np.arange(n), y_all, test_size=0.2, random_state=42, stratify=y_all)
        aug = dict(trim=trimmer, reverb=(rv, frontend.reverb_plan(n, rv.n_rows, prob=0.5, seed=4)),
                   corrupt=(mixer, frontend.mix_plan(n, 4, N, (5.0, 15.0), max_shift=1600, seed=4)), mask=chain["mask"])
        lines.append("accuracy, synthetic 12 classes x 40 clips (noise 0.001), 80 / 20 split, ridge readout, one run, UNTUNED (SNR 5 .. 15 "
                     "dB of white noise on clips whose own background lies 50 dB down; nothing was chosen for the score):")
        X = {"trimmed, clean": pipeline.features_from_utterances(clips, fe, net, None, trim=trimmer),
             "trimmed, chain": pipeline.features_from_utterances(clips, fe, net, None, **aug)}
        for train, test in (("trimmed, clean", "trimmed, clean"), ("trimmed, chain", "trimmed, chain"), ("trimmed, chain", "trimmed, clean"),
                            ("trimmed, clean", "trimmed, chain")):
            scaler = ro.StandardScaler()
            model = ro.RidgeReadout(1.0).fit(scaler.fit_transform(X[train][torch.from_numpy(i_tr).cuda()]),
                                             torch.from_numpy(y_tr).to(fe.device))
            acc = float((model.predict(scaler.transform(X[test][torch.from_numpy(i_te).cuda()])).cpu().numpy() == y_te).mean())
            lines.append(f"  trained on {train}, tested on {test}: test accuracy {100 * acc:6.2f} %")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
