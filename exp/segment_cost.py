"""What reading a launch per time segment costs (profiles/segment_features.txt).

Reservoir kernel alone, one process, at the batch sizes of bench.py's configs (rasters from the gammatone front end on the
config's audio, the reservoir built the way bench.py builds it), segment length S = T / 4:
  * the stateless launch (`run_batch`), for scale;
  * the unsegmented continued launch (`run_batch(state=...)`, lsm_reservoir_run_from);
  * the segmented launch (`run_segment_records`, lsm_reservoir_run_segments), same state;
  * the segmented launch + the window kernel (`run_segments`: per-segment rows);
  * the emulation without the feature: one `run_batch(state=...)` per segment, the feature records of the state block
    zeroed by hand and the step count set back to 0 in between, so that each launch's row is the segment's own.
HIP events around each whole form, `--runs` of every form alternating after one warm-up round.  Before any timing the
per-segment rows of the segmented launch are checked for byte equality with the emulation's, and its state with the
unsegmented launch's.

    python exp/segment_cost.py [--runs 9] [cfg2 cfg4 ...]
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
        S = t // 4
        keys = bench.FEATURE_SET
        print(f"== {name}: N={cfg['N']} n_out={cfg['n_out']} clips={clips} steps={t} S={S}, plan {net.plan(clips, t, 0)}",
              flush=True)
        np_ = (cfg["N"] + 63) // 64 * 64
        off_feat = 16 + 6 * np_ + np_ // 4
        state = net.new_state(clips)

        def fresh():
            state.data.zero_()
            state.steps_done = 0
            return state

        def emulation():
            st = fresh()
            rows = []
            for g in range(4):
                st.data[:, off_feat:].zero_()
                st.steps_done = 0
                rows.append(net.run_batch(rasters[:, :, g * S:(g + 1) * S], keys, state=st)[0])
            return torch.stack(rows, dim=1)

        forms = {"stateless launch": lambda: net.run_batch(rasters, keys)[0],
                 "run_from, unsegmented": lambda: net.run_batch(rasters, keys, state=fresh())[0],
                 "segmented launch": lambda: net.run_segment_records(rasters, S, keys, state=fresh())[0],
                 "segmented + window kernel": lambda: net.run_segments(rasters, S, keys, state=fresh()),
                 "4 launches, emulation": emulation}
        rows = forms["segmented + window kernel"]()
        seg_state = state.data.clone()
        assert torch.equal(rows, emulation()), f"{name}: segment rows differ from the four-launch emulation"
        forms["run_from, unsegmented"]()
        assert torch.equal(state.data, seg_state), f"{name}: state after the segmented launch differs"
        torch.cuda.synchronize()
        times = {label: [] for label in forms}
        for i in range(args.runs + 1):
            for label, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i:                                       # round 0 warms up
                    times[label].append(e0.elapsed_time(e1))
        base = statistics.median(times["run_from, unsegmented"])
        for label, ms in times.items():
            med = statistics.median(ms)
            print(f"   {label:28s} median {med:7.3f} ms  min {min(ms):7.3f}  max {max(ms):7.3f}  "
                  f"({med - base:+7.3f} ms, {med / base:5.3f} x run_from)", flush=True)


if __name__ == "__main__":
    main()
