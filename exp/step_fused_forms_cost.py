"""Writes the machine-made parts of profiles/step_fused_forms.txt (`--out`; printed as well).

The code objects (`--parent-tree DIR`, a checkout of the parent commit; needs hipcc, no GPU; `--no-timing` stops here):
csrc/step_fused.hip and csrc/lif_dense_{0,1,2,3}.hip of both trees compiled to assembly with the build's flags, every kernel
of the parent compared with the kernel of the same symbol in this tree, instruction for instruction and register figure for
register figure, and both tables of per-kernel resources (VGPRs, SGPRs, LDS, scratch) of the fused step: the parent's six
forms beside this tree's, and the twelve new forms of csrc/step_fused_masked.hip and csrc/step_fused_ragged.hip.

The cost (`--parent-tree DIR` with a built library in it): with GPU_MAX_HW_QUEUES=4, cfg2 of bench.py (256 clips, 128
gammatone filters, N = 1000) and `--steps` steps per measurement, one fresh process per measurement, the parent checkout and
this tree alternating, `--rounds` times over; medians and ranges of the rounds.
  plain      `HotPath.submit(audio)`: the plain fused step in both trees (control)
  masked     `submit(audio, mask=plan)`: the parent's two launches against this tree's `HotPath(fused_forms=True)`
  mixmask    the same with a mixer configured and `mix=` on every step
  ragged     `features_from_utterances` over 4096 utterances of 0.3 to 1.0 s (batches of 1024): the parent's two launches per
             batch against this tree's `fused=True`
  bench      `python bench.py --gpus 1 --steps STEPS --warmup 12` of either tree (control)
A measurement of this tree with the switch off (`two`) runs beside the others, so that the parent's route and this tree's
unchanged default stand next to each other."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit (built, for the timing)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--what", default="plain,masked,mixmask,ragged,bench", help="comma-separated measurements")
ap.add_argument("--no-timing", action="store_true", help="the code objects only (no GPU needed)")
ap.add_argument("--no-code", action="store_true", help="the timing only")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)        # one measurement in this process
ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
ap.add_argument("--route", default="two", help=argparse.SUPPRESS)
args = ap.parse_args()
lines = []
META = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


# ---- one measurement, in a process of its own ------------------------------------------------------------------------------
def child():
    sys.path.insert(0, args.tree)
    import torch
    import bench
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir, snn
    assert os.path.realpath(os.path.dirname(pipeline.__file__)).startswith(os.path.realpath(args.tree))
    cfg = bench.CONFIGS["cfg2"]
    B = cfg["batch"]
    fe = frontend.SpikeFrontEnd(cfg["n_filters"], cfg["filterbank"])
    audio_np = bench.make_audio(cfg["audio"], B, seed=1234)
    audio = torch.from_numpy(audio_np).cuda()
    wc = bench.w_critico(cfg["k"], 2.0, 2, fe.encode(audio))
    params = reservoir.SimulationParams(num_neurons=cfg["N"], num_output_neurons=cfg["n_out"], small_world_graph_k=cfg["k"],
                                        mean_weight=wc * bench.MULTIPLIER)
    net = snn.SNN(params, reservoir=reservoir.build_reservoir(params, fe.n_channels))
    fused = args.route == "fused"
    out = {"what": args.child, "route": args.route, "hw_queues": pipeline.configure_hardware_queues()}
    if args.child == "ragged":
        rs = np.random.RandomState(11)
        utts = [audio_np[i % B, :n].copy() for i, n in enumerate(rs.randint(4800, 16001, size=4096))]
        kw = {"fused": True} if fused else {}
        pipeline.features_from_utterances(utts[:1024], fe, net, bench.FEATURE_SET, batch=1024, **kw)        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = pipeline.features_from_utterances(utts, fe, net, bench.FEATURE_SET, batch=1024, **kw)
        torch.cuda.synchronize()
        out["ms"] = (time.perf_counter() - t0) * 1e3
        out["checksum"] = float(rows.double().sum())
    else:
        mixer = plan = None
        if args.child == "mixmask":
            noise = (np.random.default_rng(62).standard_normal((8, 32000)) * 0.05).astype(np.float32)
            mixer = frontend.NoiseMixer(noise)
            plan = frontend.mix_plan(B, 8, 32000, (0.0, 20.0), max_shift=1600, level_db=(-6.0, 0.0), seed=9)
        kw = {"fused_forms": True} if fused else {}
        hp = pipeline.HotPath(fe, net, bench.FEATURE_SET, mixer=mixer, **kw)
        extra = {}
        if args.child in ("masked", "mixmask"):
            extra["mask"] = frontend.mask_plan(B, fe.n_filters, fe.time_bins, freq_masks=2, freq_width=15, time_masks=2,
                                               time_width=20, seed=3)
        if plan is not None:
            extra["mix"] = plan
        calls = []
        real = pipeline.step_fused
        pipeline.step_fused = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        for _ in range(24):                                          # every stream, its buffers and the clock
            hp.submit(audio, **extra)
        hp.synchronize()
        calls.clear()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            rows, _ = hp.submit(audio, **extra)
        hp.synchronize()
        out["ms"] = (time.perf_counter() - t0) * 1e3 / args.steps
        out["fused_launches"] = len(calls)
        out["checksum"] = float(rows.double().sum())
    print("RESULT " + json.dumps(out))


# ---- the code objects ------------------------------------------------------------------------------------------------------
def assembly(tree, unit, tmp):
    import shutil
    sys.path.insert(0, ROOT)
    from lsm_speech_classifier_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(tmp, f"{abs(hash(tree))}_{unit}.s")
    subprocess.check_call([hipcc] + build.CFLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S",
                                                    os.path.join(tree, "lsm-speech-classifier_amd", "csrc", unit + ".hip"),
                                                    "-o", out], stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """symbol -> (instruction lines, register figures) of every function in an assembly file (exp/mask_cost.py)."""
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


def short(symbol):
    m = re.match(r"^_ZN12_GLOBAL__N_1\d+(step_fused\w*?_kernel_sl\d)ILi3ELb1ELi1ELb([01])ELb1EEE", symbol)
    return f"{m.group(1)}<shb0={m.group(2)}>" if m else symbol[:60]


def table(title, body, meta):
    lines.append(title)
    lines.append(f"    {'kernel':44s} {'lines':>6s} {'VGPRs':>5s} {'SGPRs':>5s} {'LDS':>4s} {'scratch':>7s}")
    for k in sorted(body):
        if "step_fused" in k and k in meta:
            v = meta[k]
            lines.append(f"    {short(k):44s} {len(body[k]):6d} {v['next_free_vgpr']:>5s} {v['next_free_sgpr']:>5s} "
                         f"{v['group_segment_fixed_size']:>4s} {v['private_segment_fixed_size']:>7s}")


def code_objects():
    from lsm_speech_classifier_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        lines.append("kernels of the parent commit against the kernels of the same symbol in this tree (hipcc "
                     + " ".join(build.CFLAGS) + "):")
        for unit in ("step_fused", "lif_dense_0", "lif_dense_1", "lif_dense_2", "lif_dense_3"):
            (pb, pm), (nb, nm) = kernels(assembly(args.parent_tree, unit, tmp)), kernels(assembly(ROOT, unit, tmp))
            same = [k for k in pb if k in nb and pb[k] == nb[k] and pm.get(k) == nm.get(k)]
            lines.append(f"  csrc/{unit}.hip: {len(pb)} kernels in the parent, {len(same)} identical instruction for instruction "
                         f"and register figure for register figure, {len(pb) - len(same)} differing; "
                         f"{sum(len(v) for v in pb.values())} instruction lines compared; new in this tree: "
                         f"{sorted(set(nb) - set(pb)) or 'none'}")
            for k in pb:
                if k not in same:
                    lines.append(f"    DIFFERS: {k} ({len(pb[k])} -> {len(nb.get(k, []))} lines, {pm.get(k)} -> {nm.get(k)})")
            if unit == "step_fused":
                table("  the six forms of the plain step, parent commit:", pb, pm)
                table("  the six forms of the plain step, this tree:", nb, nm)
        for unit in ("step_fused_masked", "step_fused_ragged"):
            b, m = kernels(assembly(ROOT, unit, tmp))
            table(f"  csrc/{unit}.hip (__launch_bounds__(256, 4): at most 128 VGPRs; LDS is dynamic, step_lds_bytes):", b, m)
            lines.append(f"    scratch bytes over the {len(m)} forms: {sorted(set(v['private_segment_fixed_size'] for v in m.values()))}")


# ---- the alternating run ---------------------------------------------------------------------------------------------------
def measure(tree, what, route):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    if what == "bench":
        cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", "12"]
        p = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} ended with {p.returncode}: {p.stderr[-2000:]}")
        d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        return {"ms": float(d.get("ms_per_step", d.get("value", float("nan")))), "line": d}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--tree", tree, "--route", route, "--steps", str(args.steps)]
    p = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:                       # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(f"{' '.join(cmd)} ended with {p.returncode}: {p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def timing():
    parent = os.path.abspath(args.parent_tree)
    lines.append(f"GPU_MAX_HW_QUEUES=4, cfg2 (256 clips, 128 gammatone filters, N = 1000), {args.steps} steps per measurement, one "
                 f"process each, parent checkout and this tree alternating, {args.rounds} rounds")
    for what in args.what.split(","):
        runs = [("parent, two launches", parent, "two"), ("this tree, two launches", ROOT, "two"),
                ("this tree, fused route", ROOT, "fused")]
        if what in ("plain", "bench"):
            runs = [("parent", parent, "two"), ("this tree", ROOT, "two")]
        got = collections.defaultdict(list)
        sums = {}
        for rnd in range(1, args.rounds + 1):
            for name, tree, route in runs:
                r = measure(tree, what, route)
                got[name].append(r["ms"])
                sums.setdefault(name, r.get("checksum"))
                note = f", {r['fused_launches']} fused launches" if "fused_launches" in r else ""
                lines.append(f"  {what:8s} round {rnd}: {name:24s} {r['ms']:9.3f} ms{note}")
                print(lines[-1], file=sys.stderr, flush=True)          # progress, while the rounds run
        unit = "ms per call" if what == "ragged" else "ms per step"
        for name, v in got.items():
            lines.append(f"  {what:8s} {name:24s} median {np.median(v):9.3f} {unit}, range {min(v):.3f} .. {max(v):.3f}"
                         + (f", checksum {sums[name]!r}" if sums[name] is not None else ""))
        if len(runs) == 3:
            p, f = got[runs[0][0]], got[runs[2][0]]
            verdict = "ON" if np.median(f) < np.median(p) and max(f) < min(p) else "OFF"
            lines.append(f"  {what:8s} rule (median lower than the parent's and the two ranges apart): switch {verdict}")


if args.child:
    child()
    sys.exit(0)
sys.path.insert(0, ROOT)
try:
    if args.parent_tree and not args.no_code:
        code_objects()
    if not args.no_timing:
        if not args.parent_tree:
            raise SystemExit("the timing alternates with a built checkout of the parent commit: --parent-tree DIR")
        timing()
finally:                                        # what was measured before a child failed is kept
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
