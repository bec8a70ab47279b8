"""What the streaming ridge fit costs (profiles/ridge_fit.txt).

  * --resources: registers, LDS and scratch of the fit kernel, from the compiler's metadata (compiles csrc/fit.hip with the
    build's flags into a temporary directory; needs hipcc, no GPU).
  * a push (`lsm_fit_accumulate_f32`) of 256 x 2000 at 12 and at 35 classes and of 1024 x 16000 at 12 classes: HIP events
    around `--iters` back-to-back pushes of one shape, the shapes alternating, `--runs` rounds after one warm-up round; medians
    with ranges, and the share of the derived floor reached (multiply-adds of the triangle's tiles at 64 float64 FMA per clock
    and CU, 256 CUs, 2.4 GHz -- a data-sheet figure, not a measurement).
  * the route end to end at cfg2 (128 gammatone filters, 1000 neurons, 400 output neurons, 5 keys, 256 clips per step, 20
    steps) against the parent's: `features_from_audio` keeping every row, then `StandardScaler.fit_transform` +
    `RidgeReadout.fit`, against `fit_from_audio` + `RidgeStatistics.solve`; host clock around calls that end in a
    synchronise, alternating, medians; the 20 steps alone give the per-step cost of the pushes inside `HotPath` with the
    hardware queues in force (GPU_MAX_HW_QUEUES); and the bytes each route holds when it solves.

    python exp/ridge_fit_cost.py [--runs 5] [--iters 10] [--resources] [--skip-large]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import numpy as np

KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']
TILE = 64


def resources():
    from lsm_speech_classifier_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc"] + build.CFLAGS + ["-I", os.path.join(build.ROOT, "include"), "-save-temps=obj", "-c",
                                          os.path.join(build.PKG_DIR, "csrc", "fit.hip"), "-o", os.path.join(tmp, "fit.o")]
        subprocess.check_call(cmd)
        asm = open([os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith("gfx950.s")][0]).read()
    for name in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
                 ".private_segment_fixed_size"):
        value = re.search(re.escape(name) + r":\s*(\d+)", asm).group(1)
        print(f"   fit_kernel {name[1:]:28s} {value}")
    print(f"   v_fmac_f64 / v_fma_f64 in the kernel: {len(re.findall(r'v_fma(c)?_f64', asm))}; "
          f"ds_read_b128: {len(re.findall(r'ds_read_b128', asm))}")


def summarise(label, ms, note=""):
    med = statistics.median(ms)
    print(f"   {label:52s} median {med:9.4f} ms  min {min(ms):9.4f}  max {max(ms):9.4f}{note}", flush=True)
    return med


def floor_us(n_rows, D):
    nt = -(-D // TILE)
    return n_rows * (nt * (nt + 1) // 2) * TILE * TILE / (64 * 256 * 2.4e9) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1024 x 16000 push (a 2 GB Gram)")
    args = ap.parse_args()
    if args.resources:
        return resources()
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline, readout, reservoir as R, snn

    # ---- a push alone ---------------------------------------------------------------------------------------------------------
    shapes = [(256, 5, 400, 12), (256, 5, 400, 35)] + ([] if args.skip_large else [(1024, 8, 2000, 12)])
    cases = []
    for n, n_keys, n_out, C in shapes:
        rng = np.random.default_rng(n + C)
        x = torch.from_numpy((rng.integers(0, 40, (n, n_keys * n_out)) * rng.choice([0.0, 1.0, 0.37, 11.5], (n, n_keys * n_out)))
                             .astype(np.float32)).cuda()
        y = torch.from_numpy(rng.integers(0, C, n).astype(np.int32)).cuda()
        cases.append((f"push {n} x {n_keys * n_out}, {C} classes", readout.RidgeStatistics([f"k{i}" for i in range(n_keys)], n_out, C, "cuda"),
                      x, y))
    times = {label: [] for label, *_ in cases}
    for i in range(args.runs + 1):
        for label, stats, x, y in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                stats.push(x, y)
            e1.record()
            e1.synchronize()
            if i:                                           # round 0 warms up
                times[label].append(e0.elapsed_time(e1) / args.iters)
    for (label, stats, x, y) in cases:
        fl = floor_us(x.shape[0], x.shape[1])
        med = statistics.median(times[label])
        summarise(label, times[label], f"  derived floor {fl:8.1f} us: {100 * fl / (med * 1e3):5.1f} % of it reached")
    del cases
    torch.cuda.empty_cache()

    # ---- the route at cfg2 against the parent's ---------------------------------------------------------------------------------
    B, steps, C = 256, 20, 12
    fe = frontend.SpikeFrontEnd(128, "gammatone")
    p = R.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=200, mean_weight=0.012)
    net = snn.SNN(p, reservoir=R.build_reservoir(p, fe.n_channels))
    rng = np.random.RandomState(3)
    t = np.arange(fe.n_samples) / fe.n_samples
    audio = np.stack([(rng.standard_normal(fe.n_samples) * 0.3 * 10.0 ** (-2.5 * np.abs(t - rng.uniform(0.3, 0.7))))
                      .astype(np.float32) for _ in range(B * steps)])
    labels = (np.arange(B * steps) % C).astype(np.int32)
    y_dev = torch.from_numpy(labels).cuda()
    print(f"== cfg2: {steps} steps of {B} clips, {len(KEYS)} keys x 400 = 2000 features, {C} classes, "
          f"{pipeline.configure_hardware_queues()} hardware queues", flush=True)

    def parent(solve=True):
        rows = pipeline.features_from_audio(audio, fe, net, KEYS, batch=B, device_out=True)
        if not solve:
            return rows, rows.numel() * 4
        scaler = readout.StandardScaler()
        clf = readout.RidgeReadout(1.0).fit(scaler.fit_transform(rows), y_dev)
        return clf, rows.numel() * 4

    def streamed(solve=True):
        stats = readout.RidgeStatistics(KEYS, 400, C, "cuda")
        pipeline.fit_from_audio(audio, labels, fe, net, KEYS, stats, batch=B)
        held = sum(t.numel() * t.element_size() for t in stats._fields()) + pipeline.FIT_ROW_BUFFERS * B * 2000 * 4
        return (stats.solve(1.0) if solve else stats), held

    forms = {"parent: 20 steps keeping rows": lambda: parent(False), "streamed: 20 steps with pushes": lambda: streamed(False),
             "parent: steps + StandardScaler + RidgeReadout.fit": parent, "streamed: steps + pushes + solve": streamed}
    wall, held = {label: [] for label in forms}, {}
    for i in range(args.runs + 1):
        for label, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, held[label] = fn()
            torch.cuda.synchronize()
            if i:
                wall[label].append((time.perf_counter() - t0) * 1e3)
    for label in forms:
        med = summarise(label, wall[label])
        print(f"      -> {med / steps:7.4f} ms per step; holds {held[label] / 2 ** 20:6.1f} MiB of rows or statistics "
              f"(float32 rows; the stored-rows fit makes float64 copies of them on top)", flush=True)
    a, b = statistics.median(wall["parent: 20 steps keeping rows"]), statistics.median(wall["streamed: 20 steps with pushes"])
    print(f"   the pushes add {(b - a) / steps:+.4f} ms to a step of {a / steps:.4f} ms", flush=True)


if __name__ == "__main__":
    main()
