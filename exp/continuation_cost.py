"""What cutting a run into continued launches costs (profiles/reservoir_state.txt).

Reservoir kernel alone, one process, at the batch sizes of bench.py's configs: rasters from the gammatone front end on the
config's audio, the reservoir built the way bench.py builds it.  One launch over the clip's 400 steps (the stateless kernel,
`run_batch`) against the same clip as 1, 4 and 8 continued launches (`run_batch(state=...)`: 1 x 400, 4 x 100, 8 x 50);
HIP events around each whole run, `--runs` of every form alternating after one warm-up round.  Feature rows are checked
for byte equality with the single launch before any timing.  Also prints the state bytes per clip of every config.

    python exp/continuation_cost.py [--runs 9] [cfg2 cfg4 ...]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

import bench
from lsm_speech_classifier_amd import frontend, reservoir as R, snn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg2", "cfg4"])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--state-bytes-only", action="store_true")
    args = ap.parse_args()
    for name in args.configs:
        cfg = bench.CONFIGS[name]
        clips = cfg["batch"]
        fe = frontend.SpikeFrontEnd(cfg["n_filters"], cfg["filterbank"])
        audio = torch.from_numpy(bench.make_audio(cfg["audio"], clips, 1234)).cuda()
        rasters = fe.encode(audio)
        wc = bench.w_critico(cfg["k"], 2.0, 2, rasters)
        p = R.SimulationParams(num_neurons=cfg["N"], num_output_neurons=cfg["n_out"], small_world_graph_k=cfg["k"],
                               mean_weight=wc * bench.MULTIPLIER)
        net = snn.SNN(p, reservoir=R.build_reservoir(p, fe.n_channels))
        t = fe.n_steps
        print(f"== {name}: N={cfg['N']} n_out={cfg['n_out']} clips={clips} steps={t} state bytes per clip "
              f"{net.state_bytes()} ({net.state_bytes() * clips / 1e6:.2f} MB per batch), plan {net.plan(clips, t, 0)}", flush=True)
        if args.state_bytes_only:
            continue

        def continued(parts):
            state = net.new_state(clips)
            feats = None
            for t0, n in snn.split_steps(t, t // parts):
                feats = net.run_batch(rasters[:, :, t0:t0 + n], bench.FEATURE_SET, state=state)[0]
            return feats

        forms = {"1 launch, no state": lambda: net.run_batch(rasters, bench.FEATURE_SET)[0],
                 "1 x 400 continued": lambda: continued(1), "4 x 100 continued": lambda: continued(4),
                 "8 x 50 continued": lambda: continued(8)}
        ref = forms["1 launch, no state"]()
        for label, fn in forms.items():
            assert torch.equal(fn(), ref), f"{name}: {label} differs from the single launch"
        torch.cuda.synchronize()
        times = {label: [] for label in forms}
        for _ in range(args.runs):
            for label, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[label].append(e0.elapsed_time(e1))
        base = statistics.median(times["1 launch, no state"])
        for label, ms in times.items():
            med = statistics.median(ms)
            print(f"   {label:22s} median {med:7.3f} ms  min {min(ms):7.3f}  max {max(ms):7.3f}  ({med / base:5.3f} x the single launch)",
                  flush=True)


if __name__ == "__main__":
    main()
