"""Writes profiles/spec_mask.txt's two machine-made parts (`--out`; printed as well).

The code objects (`--parent-tree DIR`, a checkout of the parent commit; needs hipcc, no GPU; `--no-timing` stops here):
csrc/frontend.hip and csrc/mel.hip of both trees compiled to assembly with the build's flags, and every kernel of the
parent compared with the kernel of the same symbol in this tree -- instruction for instruction (labels renumbered, comments
and debug directives dropped) and register count for register count (next_free_vgpr / next_free_sgpr / accum_offset, LDS,
scratch).  csrc/mask.hip's kernels are listed with their register counts beside their unmasked twins'.

The cost: the fused gammatone launch for 256 clips x 128 filters with the hardware-queue count the machine sets, timed with
device events in ONE process, alternating: the unmasked launch of a parent build (`--parent-lib`, loaded beside this
tree's library), the unmasked launch of this tree, the masked launch of this tree (plan: 2 frequency masks up to 15 wide,
2 time masks up to 20 wide).  Medians of 20 after 4 warm-up launches, `--rounds` times over, so that the spread between
equal rounds stands beside the differences."""
import argparse
import collections
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit: compare the kernels' code")
ap.add_argument("--parent-lib", default=None, help="liblsm_hip.so built from the parent commit: time its unmasked launch")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-timing", action="store_true", help="the code objects only (no GPU needed)")
args = ap.parse_args()
lines = []
META = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def assembly(tree, unit, tmp):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(tmp, f"{abs(hash(tree))}_{unit}.s")
    subprocess.check_call([hipcc] + build.CFLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S",
                                                    os.path.join(tree, "lsm-speech-classifier_amd", "csrc", unit + ".hip"),
                                                    "-o", out], stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """symbol -> (instruction lines, register figures) of every function in an assembly file."""
    body, meta, cur, lines_, name = {}, collections.defaultdict(dict), None, [], None
    for raw in open(path):
        s = raw.rstrip("\n")
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", s)
        if m and cur is None:
            cur, lines_ = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", s):
                body[cur], cur = lines_, None
                continue
            t = s.split(";")[0].strip()
            if t and not t.startswith((".p2align", ".loc", ".cfi")):
                lines_.append(re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"\.LBB\d+_", ".LBB_", t)))
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            name = m.group(1)
        m = re.match(r"^\s*\.amdhsa_(%s)\s+(\S+)" % "|".join(META), s)
        if m:
            meta[name][m.group(1)] = m.group(2)
    return body, meta


def code_objects():
    with tempfile.TemporaryDirectory() as tmp:
        lines.append("kernels of the parent commit against the kernels of the same symbol in this tree (hipcc "
                     + " ".join(build.CFLAGS) + "):")
        mine = {}
        for unit in ("frontend", "mel"):
            (pb, pm), (nb, nm) = kernels(assembly(args.parent_tree, unit, tmp)), kernels(assembly(ROOT, unit, tmp))
            mine[unit] = (nb, nm)
            same = [k for k in pb if k in nb and pb[k] == nb[k] and pm.get(k) == nm.get(k)]
            lines.append(f"  csrc/{unit}.hip: {len(pb)} kernels in the parent, {len(same)} identical instruction for instruction "
                         f"and register count for register count, {len(pb) - len(same)} differing; "
                         f"{sum(len(v) for v in pb.values())} instruction lines compared; new in this tree: "
                         f"{sorted(set(nb) - set(pb)) or 'none'}")
            for k in pb:
                if k not in same:
                    lines.append(f"    DIFFERS: {k} ({len(pb[k])} -> {len(nb.get(k, []))} lines, {pm.get(k)} -> {nm.get(k)})")
        mb, mm = kernels(assembly(ROOT, "mask", tmp))
        fb, fm = mine["frontend"]
        lines.append(f"  csrc/mask.hip: {len(mb)} kernels; scratch bytes: {sorted(set(v['private_segment_fixed_size'] for v in mm.values()))}")
        lines.append("  masked kernel: instruction lines / VGPRs / SGPRs (its unmasked twin's)")
        for k in sorted(mb):
            twin = k.replace("30gammatone_spikes_masked_kernel", "23gammatone_spikes_kernel").replace(
                "28spec_to_spikes_masked_kernel", "21spec_to_spikes_kernel").replace("N6lsm_fe8MaskArgsE", "")
            twin = next((t for t in fb if t.startswith(twin[:-1])), None)
            short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", k)[:52]
            lines.append(f"    {short:52s} {len(mb[k]):6d} / {mm[k]['next_free_vgpr']:>3s} / {mm[k]['next_free_sgpr']:>3s}"
                         + (f"   ({len(fb[twin])} / {fm[twin]['next_free_vgpr']} / {fm[twin]['next_free_sgpr']})" if twin else ""))


if args.parent_tree:
    code_objects()

if not args.no_timing:
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, synth

    lib = _lib.load()
    _lib.require_gpu()
    B, F = 256, 128
    fe = frontend.SpikeFrontEnd(F, "gammatone")
    lines += [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}",
              f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}: layout of {B} clips x {F} filters = "
              f"{lib.lsm_gammatone_spikes_layout(B, F, 0)} (0 lane pair, 1 / 2 chains per lane)"]
    audio = torch.from_numpy(synth.class_chirps(np.arange(B) % 12, seed=5)).cuda()
    on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
    ws = fe.new_workspace(B)
    raster = torch.empty((B, fe.n_channels, fe.n_steps), dtype=torch.uint8, device="cuda")
    plan = frontend.mask_plan(B, F, fe.time_bins, freq_masks=2, freq_width=15, time_masks=2, time_width=20, seed=3)
    fmask, tmask = frontend.upload_mask(plan, B, F, fe.time_bins, fe.device)
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda t: C.c_void_p(t.data_ptr())
    host = lambda a: C.c_void_p(a.ctypes.data)
    head = (void(audio), B, fe.n_samples, void(fe.coefs), F, fe.nwin, fe.hop, fe.ncols, fe.time_bins, host(on), host(off),
            len(on), fe.redundancy, void(raster), void(ws), ws.numel() * 8, fe.coef_flags, 0)

    def launcher(fn, *tail):
        def go():
            assert fn(*head, *tail, stream) == 0
        return go

    forms = [("this tree, unmasked", launcher(lib.lsm_gammatone_spikes_f64)),
             ("this tree, masked  ", launcher(lib.lsm_gammatone_spikes_masked_f64, void(fmask), void(tmask)))]
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.lsm_gammatone_spikes_f64.restype, parent.lsm_gammatone_spikes_f64.argtypes = _lib._SIGS["lsm_gammatone_spikes_f64"]
        parent.lsm_build_id.restype = C.c_char_p
        lines.append(f"parent build: {parent.lsm_build_id().decode()}")
        forms.insert(0, ("parent,    unmasked", launcher(parent.lsm_gammatone_spikes_f64)))

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
    for name, v in med.items():
        lines.append(f"  {name}: median of the rounds {np.median(v):8.1f} us, rounds between {min(v):.1f} and {max(v):.1f} "
                     f"(spread {max(v) - min(v):.1f} us)")
    forms[-2][1]()
    torch.cuda.synchronize()
    plain = raster.clone()
    forms[-1][1]()
    torch.cuda.synchronize()

    def bits(words, n):
        i = np.arange(n)
        return ((words[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)
    cells = (bits(plan.freq, F)[:, :, None] | bits(plan.time, fe.time_bins)[:, None, :]).sum(axis=(1, 2))
    lines.append(f"  masked cells per clip: {cells.mean():.0f} of {F * fe.time_bins} on average; clips whose raster the mask "
                 f"changed: {int((raster != plain).flatten(1).any(1).sum())} of {B}")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
