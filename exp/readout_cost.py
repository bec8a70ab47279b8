"""What the labels of a stream push cost (profiles/readout.txt).

256 streams, 5 keys x 400 output neurons, windows of 10 segments, hop 1, pushes of 10 segments: every stream's joined run is 19
records (9 kept + 10 new) and completes 10 windows, 2560 rows of 2000 features.  Two models, 12 and 35 classes.  Timed:
  * fused: one `lsm_readout_windows` launch (`DeviceReadout.score_windows`) -- records in, logits and labels out;
  * parent route: `lsm_segment_features_ragged` (`SNN.segment_features(segments=...)`), then the scaler, the matmul and the
    argmax in torch, float64 -- what a caller had to write before;
  * for scale, the parent route's feature launch alone and `lsm_readout_rows_f32` on its rows.
HIP events around `--iters` back-to-back calls of one form, the forms alternating, `--runs` rounds after one warm-up round;
medians with ranges.  Before any timing the fused logits are checked against the torch route's within the summation bound
and the labels for equality where the top-two margin is clear.  Then the share of a whole `AudioStreamBank` push (one second
of audio per stream through the gammatone stream, the reservoir and either route) that the labels are: host clock around
pushes that end in a synchronise.

    python exp/readout_cost.py [--runs 5] [--iters 20]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from lsm_speech_classifier_amd import frontend, pipeline, readout, reservoir as R, snn, synth

KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']
B, N, N_OUT, F, S, K, H, G_NEW = 256, 1000, 400, 128, 40, 10, 1, 10


def model_for(n_classes, rows, seed):
    """A ridge readout fitted on the rows themselves (random labels): realistic magnitudes of mean, scale and coef."""
    x = rows.reshape(-1, rows.shape[-1])
    y = torch.from_numpy(np.random.default_rng(seed).integers(0, n_classes, len(x))).to(x.device)
    y[:n_classes] = torch.arange(n_classes, device=x.device)
    scaler = readout.StandardScaler().fit(x)
    clf = readout.RidgeReadout(1.0).fit(scaler.transform(x), y)
    return readout.LinearModel.from_fitted(scaler, clf, KEYS, N_OUT)


def summarise(label, ms, base=None):
    med = statistics.median(ms)
    tail = f"  ({med / base:5.2f} x fused)" if base else ""
    print(f"   {label:44s} median {med:8.4f} ms  min {min(ms):8.4f}  max {max(ms):8.4f}{tail}", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    raster = synth.bernoulli_raster(B, F, (K - 1 + G_NEW) * S, 0.2, seed=1)
    p = R.SimulationParams(num_neurons=N, num_output_neurons=N_OUT, small_world_graph_k=200, mean_weight=0.012)
    net = snn.SNN(p, reservoir=R.build_reservoir(p, F))
    G = K - 1 + G_NEW
    records, _, _ = net.run_stream_records(raster, S)
    have = torch.full((B,), G, dtype=torch.int32, device="cuda")
    rows = net.segment_features(records, S, KEYS, K, H, segments=have)
    print(f"== {B} streams, {len(KEYS)} keys x {N_OUT} neurons, {G} records per stream, {rows.shape[1]} windows each: "
          f"{rows.shape[0] * rows.shape[1]} rows of {rows.shape[2]} features; mean spikes per record "
          f"{float((records[..., 0] & 0xFFFF).float().mean()):.2f}", flush=True)
    for n_classes in (12, 35):
        model = model_for(n_classes, rows, seed=n_classes)
        ro = readout.DeviceReadout(model, "cuda")

        def fused():
            return ro.score_windows(net, records, S, K, H, segments=have)

        def features_only():
            return net.segment_features(records, S, KEYS, K, H, segments=have)

        def parent():
            x = net.segment_features(records, S, KEYS, K, H, segments=have)
            z = (x.to(torch.float64) - ro.mean) / ro.scale
            logits = z @ ro.coef.T + ro.intercept
            return logits, logits.argmax(dim=-1)

        def rows_launch():
            return ro.score_rows(rows)

        lg_f, lb_f = fused()
        lg_p, lb_p = parent()
        torch.cuda.synchronize()
        flat = rows.reshape(-1, rows.shape[-1]).cpu().numpy()
        z = (flat.astype(np.float64) - model.mean) / model.scale
        n = z.shape[1] + 2
        g = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
        bound = 2 * g * (np.abs(model.intercept)[None] + np.abs(z) @ np.abs(model.coef).T)
        diff = np.abs(lg_f.cpu().numpy().reshape(bound.shape) - lg_p.cpu().numpy().reshape(bound.shape))
        assert (diff <= bound).all(), "fused logits outside the summation bound of the torch route"
        top = np.sort(lg_p.cpu().numpy().reshape(bound.shape), axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * bound.max(axis=1)
        assert (lb_f.cpu().numpy().reshape(-1)[clear] == lb_p.cpu().numpy().reshape(-1)[clear]).all()
        print(f"-- {n_classes} classes: logits agree within the bound (largest difference {diff.max():.3g}), labels equal on "
              f"{int(clear.sum())} of {len(clear)} rows with a clear margin", flush=True)
        forms = {"fused lsm_readout_windows": fused, "parent: features + torch f64 readout": parent,
                 "   of which lsm_segment_features_ragged": features_only, "lsm_readout_rows_f32 on existing rows": rows_launch}
        times = {label: [] for label in forms}
        for i in range(args.runs + 1):
            for label, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                if i:                                       # round 0 warms up
                    times[label].append(e0.elapsed_time(e1) / args.iters)
        base = summarise("fused lsm_readout_windows", times["fused lsm_readout_windows"])
        for label in list(forms)[1:]:
            summarise(label, times[label], base)

        # ---- the share of a whole audio push ------------------------------------------------------------------------------
        hop = frontend.STREAM_HOP
        rng = np.random.RandomState(5)
        second = (rng.standard_normal((B, 100 * hop)) * 0.1).astype(np.float32)
        probe = frontend.GammatoneStream(F, B, (-60.0, -10.0)).push(second, want_db=True)
        db = probe[2].cpu().numpy()
        lo, hi = (float(v) for v in np.percentile(db[np.isfinite(db)], (20, 80)))
        audio = torch.from_numpy(second).cuda()

        def bank(with_readout):
            return pipeline.AudioStreamBank(frontend.GammatoneStream(F, B, (lo, hi)), net, S, K, H, KEYS,
                                            readout=ro if with_readout else None)

        banks = {"push (rows only)": bank(False), "push + torch f64 readout": bank(False), "push_scores": bank(True)}

        def one(label):
            bk = banks[label]
            if label == "push_scores":
                return bk.push_scores(audio)
            x, _ = bk.push(audio)
            if label == "push + torch f64 readout" and x.shape[1]:
                zz = (x.to(torch.float64) - ro.mean) / ro.scale
                return (zz @ ro.coef.T + ro.intercept).argmax(dim=-1)
            return x

        wall = {label: [] for label in banks}
        for i in range(args.runs + 2):
            for label in banks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                one(label)
                torch.cuda.synchronize()
                if i > 1:                                   # two warm-up pushes: the second is the first with full windows
                    wall[label].append((time.perf_counter() - t0) * 1e3)
        push_ms = summarise("AudioStreamBank.push, 1 s x 256 streams (wall)", wall["push (rows only)"])
        for label in ("push + torch f64 readout", "push_scores"):
            med = summarise(f"AudioStreamBank {label} (wall)", wall[label])
            print(f"      -> the labels add {med - push_ms:+.3f} ms to a push of {push_ms:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
