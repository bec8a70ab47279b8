"""Pair blocks against quads for reservoirs with 129 to 256 input channels (profiles/pair_wide_channels.txt).

Reservoir kernel alone, one process: rasters from the gammatone front end on synth.class_chirps, the reservoir built the way
bench.py builds it, the kernel forced by name ("ring-quads" / "ring-pairs") and the two alternated; HIP events around
`run_batch` (the product's launch: longest clips first), `--launches` each after two warm-up launches.  Feature rows are
checked for byte equality before any timing.

    python exp/pair_wide_channels.py [--launches 7] [N,k,n_out,filters,clips ...]
    python exp/pair_wide_channels.py --plan-only N,k,n_out,filters,clips      # what auto and "ring" would launch
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
from lsm_speech_classifier_amd import frontend, reservoir as R, snn

DEFAULT_CASES = ["4000,800,1600,256,1024", "4000,800,1600,160,1024", "1536,300,512,200,512"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--plan-only", action="store_true")
    args = ap.parse_args()
    for case in args.cases:
        n, k, n_out, filters, clips = (int(x) for x in case.split(","))
        fe = frontend.SpikeFrontEnd(filters, "gammatone")
        audio = torch.from_numpy(bench.make_audio("class_chirps", clips, 1234)).cuda()
        rasters = fe.encode(audio)
        wc = bench.w_critico(k, 2.0, 2, rasters)
        p = R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k, mean_weight=wc * bench.MULTIPLIER)
        net = snn.SNN(p, reservoir=R.build_reservoir(p, fe.n_channels))
        t = fe.n_steps
        print(f"== N={n} k={k} n_out={n_out} filters={filters} clips={clips} steps={t} raster density "
              f"{float(rasters.float().mean()):.4f}", flush=True)
        for kernel in ("auto", "ring"):
            net.set_kernel(kernel)
            print(f"   plan[{kernel}]: {net.plan(clips, t, 0)}", flush=True)
        if args.plan_only:
            continue
        feats = {}
        for kernel in ("ring-quads", "ring-pairs"):
            net.set_kernel(kernel)
            print(f"   plan[{kernel}]: {net.plan(clips, t, 0)}", flush=True)
            for _ in range(2):
                f, _, _ = net.run_batch(rasters, bench.FEATURE_SET)
            torch.cuda.synchronize()
            feats[kernel] = f.cpu().numpy()
        same = feats["ring-quads"].tobytes() == feats["ring-pairs"].tobytes()
        print(f"   feature rows byte-equal: {same}; spikes per output neuron and clip "
              f"{float(feats['ring-quads'][:, :n_out].mean()):.2f}", flush=True)
        if not same:
            sys.exit(1)
        ms = {"ring-quads": [], "ring-pairs": []}
        for _ in range(args.launches):
            for kernel in ms:
                net.set_kernel(kernel)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                net.run_batch(rasters, bench.FEATURE_SET)
                e1.record()
                torch.cuda.synchronize()
                ms[kernel].append(e0.elapsed_time(e1))
        for kernel, v in ms.items():
            print(f"   {kernel}: median {statistics.median(v):.3f} ms, range {min(v):.3f}..{max(v):.3f} "
                  f"({', '.join(f'{x:.3f}' for x in v)})", flush=True)
        q, pr = statistics.median(ms["ring-quads"]), statistics.median(ms["ring-pairs"])
        print(f"   pairs / quads = {pr / q:.3f}", flush=True)


if __name__ == "__main__":
    main()
