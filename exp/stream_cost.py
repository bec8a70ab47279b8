"""What the stream launch costs and saves (profiles/stream_segments.txt).

Reservoir kernel alone, one process, at the batch sizes of bench.py's configs: rasters from the gammatone front end on the
config's audio, the reservoir built the way bench.py builds it; a lone launch, HIP events around each whole run, `--runs`
(odd) of every form alternating after one warm-up round, medians.  Outputs are checked for byte equality before any timing.

  segments  `run_segment_records(state=...)`, one launch over the clip's steps: the bounded segmented launch.
            Run in a checkout of the parent commit this is the parent's launch, here the same launch in this tree: what the
            existing path lost to the stream mode
  stream    `run_stream_records(state=...)`, every clip at full G: no fold of the records, no merge in the epilogue
  ragged    `run_stream_records(segments=...)`, counts drawn uniformly from [G / 4, G] (seeded), against `stream`
  ragged, index order     the same with `longest_first=False`

S = steps / 16 (G = 16) where 16 divides the steps, else steps / 4.  A tree without
`run_stream_records` (the parent commit) runs `segments` alone.  `--json` adds one machine-readable line per config.

    python exp/stream_cost.py [--runs 9] [--json] [cfg2 cfg4 ...]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import bench
from lsm_speech_classifier_amd import frontend, reservoir as R, snn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg2", "cfg4"])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    assert args.runs % 2 == 1, "an odd number of runs has a median that is one of them"
    has_stream = hasattr(snn.SNN, "run_stream_records")
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
        G = 16 if t % 16 == 0 else 4
        S = t // G
        print(f"== {name}: N={cfg['N']} n_out={cfg['n_out']} clips={clips} steps={t} S={S} G={G} plan {net.plan(clips, t, 0)}",
              flush=True)
        stats = torch.empty((clips, 2), dtype=torch.int32, device="cuda")

        def segments_run():
            return net.run_segment_records(rasters, S, stats_out=stats, state=net.new_state(clips))[0]

        forms = {"segments": segments_run}
        ref = segments_run()
        ratio = None
        if has_stream:
            counts = np.random.RandomState(4321).randint(G // 4, G + 1, size=clips)
            counts_dev = torch.from_numpy(counts.astype(np.int32)).cuda()
            ratio = float(counts.sum()) / float(clips * G)

            def stream_run(**kw):
                return net.run_stream_records(rasters, S, stats_out=stats, state=net.new_state(clips), **kw)[0]

            forms["stream"] = stream_run
            forms["ragged"] = lambda: stream_run(segments=counts_dev)
            forms["ragged, index order"] = lambda: stream_run(segments=counts_dev, longest_first=False)
            assert torch.equal(stream_run(), ref), f"{name}: the stream launch's records differ from the segmented launch's"
            rag = forms["ragged"]()
            assert torch.equal(forms["ragged, index order"](), rag), f"{name}: the start order changes the results"
            live = torch.arange(G, device="cuda")[None, :] < counts_dev[:, None]
            assert torch.equal(rag[live], ref[live]) and not rag[~live].any(), f"{name}: ragged records"
        torch.cuda.synchronize()
        for fn in forms.values():                   # one warm-up round
            fn()
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
        base = statistics.median(times["segments"])
        for label, ms in times.items():
            med = statistics.median(ms)
            print(f"   {label:22s} median {med:7.3f} ms  min {min(ms):7.3f}  max {max(ms):7.3f}  ({med / base:5.3f} x segments)",
                  flush=True)
        if ratio is not None:
            print(f"   summed segments ragged / full = {ratio:.4f}; time ragged / stream = "
                  f"{statistics.median(times['ragged']) / statistics.median(times['stream']):.4f}", flush=True)
        if args.json:
            print("JSON " + json.dumps({"config": name, "has_stream": has_stream, "segments_ratio": ratio,
                                        "median_ms": {k: statistics.median(v) for k, v in times.items()},
                                        "min_ms": {k: min(v) for k, v in times.items()},
                                        "max_ms": {k: max(v) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
