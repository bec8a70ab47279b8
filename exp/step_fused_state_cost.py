"""Writes the timing part of profiles/step_fused_state.txt (`--out`; printed as well): what the one-launch step with carried
state and time segments (include/lsm_hip_step_state.h) costs against the launches it replaces.

`--parent-tree DIR`: a built checkout of the parent commit.  With GPU_MAX_HW_QUEUES=4 and cfg2 of bench.py (256 clips, 128
gammatone filters, N = 1000), one fresh process per measurement, the parent checkout and this tree alternating, `--rounds`
times over; medians and ranges of the rounds.  Every figure is the time between two HIP events on the submitting stream,
which the pipeline's streams are forked from and joined to.
  segments   `HotPath(time_segments=4).submit(audio)` over `--steps` steps: the parent's three launches against this tree's
             `HotPath(time_segments=4, fused_forms=True)` (one launch)
  sliding    `sliding_features_from_long_audio` over 256 recordings of 4 windows (segments of 100 steps, windows of 2, hop 1):
             the parent against this tree's `fused=True`
  plain      `HotPath.submit(audio)`: the plain fused step in both trees (control: its code is unchanged)
A measurement of this tree with the switch off (`two`) runs beside the others.  The compiler part of the profile is
exp/ragged_frontend_resources.py --units (kernel by kernel against the parent) and the resource remarks of
csrc/step_fused_state.hip."""
import argparse
import collections
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--what", default="segments,sliding,plain", help="comma-separated measurements")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)        # one measurement in this process
ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
ap.add_argument("--route", default="two", help=argparse.SUPPRESS)
args = ap.parse_args()
lines = []


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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if args.child == "sliding":
        long_audio = torch.cat([audio, audio.roll(1, 0), audio.roll(2, 0), audio.roll(3, 0)], dim=1).contiguous()
        kw = {"fused": True} if fused else {}
        call = lambda: pipeline.sliding_features_from_long_audio(long_audio, fe, net, bench.FEATURE_SET, fe.n_steps // 4, 2, 1,
                                                                 **kw)
        call()                                                       # warm-up
        torch.cuda.synchronize()
        e0.record()
        rows = call()
        e1.record()
        e1.synchronize()
        out["ms"] = e0.elapsed_time(e1)
    else:
        kw = {"fused_forms": True} if fused else {}
        if args.child == "segments":
            kw["time_segments"] = 4
        hp = pipeline.HotPath(fe, net, bench.FEATURE_SET, **kw)
        calls = []
        for name in ("step_fused", "step_fused_segments"):
            real = getattr(pipeline, name, None)
            if real is not None:
                setattr(pipeline, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
        for _ in range(24):                                          # every stream, its buffers and the clock
            hp.submit(audio)
        hp.synchronize()
        calls.clear()
        e0.record()
        hp.fork_from_current()
        for _ in range(args.steps):
            rows, _ = hp.submit(audio)
        hp.join_to_current()
        e1.record()
        e1.synchronize()
        hp.synchronize()
        out["ms"] = e0.elapsed_time(e1) / args.steps
        out["fused_launches"] = len(calls)
    out["checksum"] = float(rows.double().sum())
    print("RESULT " + json.dumps(out))


def measure(tree, what, route):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--tree", tree, "--route", route, "--steps", str(args.steps)]
    p = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:                       # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(f"{' '.join(cmd)} ended with {p.returncode}: {p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def timing():
    parent = os.path.abspath(args.parent_tree)
    lines.append(f"GPU_MAX_HW_QUEUES=4, cfg2 (256 clips, 128 gammatone filters, N = 1000), {args.steps} steps per measurement, one "
                 f"process each, HIP events, parent checkout and this tree alternating, {args.rounds} rounds")
    for what in args.what.split(","):
        runs = [("parent, separate launches", parent, "two"), ("this tree, separate launches", ROOT, "two"),
                ("this tree, fused route", ROOT, "fused")]
        if what == "plain":
            runs = [("parent", parent, "two"), ("this tree", ROOT, "two")]
        got, sums = collections.defaultdict(list), {}
        for rnd in range(1, args.rounds + 1):
            for name, tree, route in runs:
                r = measure(tree, what, route)
                got[name].append(r["ms"])
                sums.setdefault(name, r.get("checksum"))
                note = f", {r['fused_launches']} fused launches" if "fused_launches" in r else ""
                lines.append(f"  {what:8s} round {rnd}: {name:30s} {r['ms']:9.3f} ms{note}")
                print(lines[-1], file=sys.stderr, flush=True)          # progress, while the rounds run
        unit = "ms per call" if what == "sliding" else "ms per step"
        for name, v in got.items():
            lines.append(f"  {what:8s} {name:30s} median {np.median(v):9.3f} {unit}, range {min(v):.3f} .. {max(v):.3f}, "
                         f"checksum {sums[name]!r}")
        if len(runs) == 3:
            p, f = got[runs[0][0]], got[runs[2][0]]
            verdict = "ON" if np.median(f) < np.median(p) and max(f) < min(p) else "OFF"
            lines.append(f"  {what:8s} rule (median lower than the parent's and the two ranges apart): switch {verdict}")


if args.child:
    child()
    sys.exit(0)
try:
    if not args.parent_tree:
        raise SystemExit("the timing alternates with a built checkout of the parent commit: --parent-tree DIR")
    timing()
finally:                                        # what was measured before a child failed is kept
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
