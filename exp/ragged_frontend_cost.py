"""Writes the timing part of profiles/ragged_frontend.txt (`--out`; printed as well).

The fused gammatone launch for 256 clips (`--clips`) x 128 filters at time_bins = 100, with the hardware-queue count the machine sets
and, `--queues 12`, with the package's own, timed with device events in ONE process, the forms alternating:
  (a) the unragged launch of this tree and of a parent build (`--parent-lib`, loaded beside this tree's library): their
      ratio is the run-to-run spread;
  (b) the ragged launch with every clip at full length;
  (c) the ragged launch with lengths uniform in 0.3 .. 1.0 s (30 .. 100 bins, seeded), clips in the order drawn and longest
      first;
  (d) the same clips grouped by length, one unragged launch per distinct length (71 at most), front ends and buffers made
      before the clock starts.
Medians of 9 after 3 warm-up launches, `--rounds` times over (default 5), so that the spread between equal rounds stands
beside the differences."""
import argparse
import collections
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--parent-lib", default=None, help="liblsm_hip.so built from the parent commit: time its unragged launch")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--queues", default=None, help="GPU_MAX_HW_QUEUES for this process (it selects the layout)")
ap.add_argument("--clips", type=int, default=256,
                help="clips per launch (default 256: one wave or lane-pair wave group per SIMD; 4096: several rounds of waves)")
args = ap.parse_args()
if args.queues:
    os.environ["GPU_MAX_HW_QUEUES"] = args.queues

import torch  # noqa: E402
from lsm_speech_classifier_amd import _lib, frontend, synth  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
B, F, TB, HOP = args.clips, 128, 100, 160
fe = frontend.SpikeFrontEnd(F, "gammatone")
lines = [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}",
         f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}: layout of {B} clips x {F} filters = "
         f"{lib.lsm_gammatone_spikes_layout(B, F, 0)} (0 lane pair, 1 / 2 chains per lane)"]
audio = torch.from_numpy(synth.class_chirps(np.arange(B) % 12, seed=5)).cuda()
on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
ws = fe.new_workspace(B)
raster = torch.empty((B, fe.n_channels, fe.n_steps), dtype=torch.uint8, device="cuda")
steps = torch.empty((B,), dtype=torch.int32, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
void = lambda t: C.c_void_p(t.data_ptr())
host = lambda a: C.c_void_p(a.ctypes.data)
shape = (void(audio), B, fe.n_samples, void(fe.coefs), F, fe.nwin, fe.hop, fe.ncols, fe.time_bins)
thr = (host(on), host(off), len(on), fe.redundancy, void(raster))
tail = (void(ws), ws.numel() * 8, fe.coef_flags, 0, stream)


def unragged(library):
    def go():
        assert library.lsm_gammatone_spikes_f64(*shape, *thr, *tail) == 0
    return go


def ragged(bins_dev):
    def go():
        assert lib.lsm_gammatone_spikes_ragged_f64(*shape, void(bins_dev), *thr, void(steps), *tail) == 0
    return go


rng = np.random.default_rng(7)
drawn = rng.integers(30, TB + 1, size=B).astype(np.int32)
full = torch.full((B,), TB, dtype=torch.int32, device="cuda")
bins_drawn = torch.from_numpy(drawn).cuda()
bins_sorted = torch.from_numpy(np.sort(drawn)[::-1].copy()).cuda()
share = float((drawn.astype(np.int64) * HOP - 80).sum()) / float(B * (TB * HOP - 80))
lines.append(f"lengths of (c) and (d): {B} draws uniform in 30 .. {TB} bins, mean {drawn.mean():.1f}, {len(set(drawn.tolist()))} "
             f"distinct; samples filtered: {share:.3f} of the full-length batch's")

# (d): one unragged front end and launch per distinct length, everything made beforehand
groups = []
for t in sorted(set(drawn.tolist()), reverse=True):
    rows = np.flatnonzero(drawn == t)
    fe_t = frontend.SpikeFrontEnd(F, "gammatone", time_bins=int(t), n_samples=HOP * int(t))
    x = audio[torch.from_numpy(rows).cuda(), :HOP * int(t)].contiguous()
    out = torch.empty((len(rows), fe_t.n_channels, fe_t.n_steps), dtype=torch.uint8, device="cuda")
    groups.append((fe_t, x, out, fe_t.new_workspace(len(rows))))


def grouped():
    for fe_t, x, out, w in groups:
        fe_t.encode(x, fused=True, raster_out=out, workspace=w)


forms = [("(a) unragged, this tree      ", unragged(lib)),
         ("(b) ragged, all full length  ", ragged(full)),
         ("(c) ragged, 0.3-1.0 s, as drawn", ragged(bins_drawn)),
         ("(c) ragged, 0.3-1.0 s, longest first", ragged(bins_sorted)),
         (f"(d) {len(groups)} unragged launches, one per length", grouped)]
if args.parent_lib:
    parent = C.CDLL(args.parent_lib)
    parent.lsm_gammatone_spikes_f64.restype, parent.lsm_gammatone_spikes_f64.argtypes = _lib._SIGS["lsm_gammatone_spikes_f64"]
    parent.lsm_build_id.restype = C.c_char_p
    lines.append(f"parent build: {parent.lsm_build_id().decode()}")
    forms.insert(0, ("(a) unragged, parent build   ", unragged(parent)))


def timed(fn, reps=9, warm=3):
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
# the full-length ragged launch writes the unragged launch's bytes
forms[-5][1]()
torch.cuda.synchronize()
plain = raster.clone()
ragged(full)()
torch.cuda.synchronize()
lines.append(f"  ragged at full length == unragged, byte for byte: {bool(torch.equal(raster, plain))}; steps all {TB * len(on)}: "
             f"{bool((steps == TB * len(on)).all())}")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
