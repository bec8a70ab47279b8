"""Times the adaptive-range encoder (profiles/adaptive_range.txt): `AdaptiveStream.push` against the inner stream's `push`
alone -- the path of the parent commit -- and `AdaptiveEncoder.push_db` by itself, on 256 streams x 128 gammatone filters and
256 streams x 40 mel filters at 10 and at 100 hops per push.  Medians of 40 pushes timed with device events after 8 warm-up
pushes (which also carry every stream past its start-up latency, so that each push completes all its columns); the two
routes alternate, twice, so that the spread between equal runs stands beside the difference."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import _lib, frontend  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
lines = [f"package at {ROOT}, build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}"]


def timed(fn, reps=40, warm=8):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), a.elapsed_time(b) * 1e3 / reps


def fmt(t):
    return f"median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f}; back to back {t[3]:.1f} us/push)"


N_STREAMS, HOP, L = 256, 160, 100
for kind, F in (("gammatone", 128), ("mel", 40)):
    for H in (10, 100):
        rng = np.random.default_rng(F + H)
        audio = torch.from_numpy((rng.standard_normal((N_STREAMS, H * HOP)) * 0.1).astype(np.float32)).cuda()

        def make():
            if kind == "gammatone":
                return frontend.GammatoneStream(F, N_STREAMS, (-60.0, -10.0))
            return frontend.MelStream(F, N_STREAMS, (-60.0, -10.0))

        inner, ads = make(), frontend.AdaptiveStream(make(), L)
        raster = torch.zeros((N_STREAMS, F, H * 4), dtype=torch.uint8, device="cuda")
        db = torch.zeros((N_STREAMS, F, H), dtype=ads.db_dtype, device="cuda")
        lines.append(f"{N_STREAMS} streams x {F} {kind} filters, {H} hops per push, window {L} columns:")
        for rnd in (1, 2):
            t_in = timed(lambda: inner.push(audio, raster_out=raster))
            t_db = timed(lambda: inner.push(audio, raster_out=raster, db_out=db))
            t_ad = timed(lambda: ads.push(audio, raster_out=raster))
            lines.append(f"  round {rnd}: inner push                 {fmt(t_in)}")
            lines.append(f"  round {rnd}: inner push with db_out     {fmt(t_db)}")
            lines.append(f"  round {rnd}: AdaptiveStream.push        {fmt(t_ad)}   added: {t_ad[0] - t_in[0]:+.1f} us = "
                         f"{(t_ad[0] - t_in[0]) / t_in[0] * 100:+.1f} % of the inner push")
        enc = frontend.AdaptiveEncoder(F, N_STREAMS, ads.db_dtype, L)
        inner.push(audio, raster_out=raster, db_out=db)
        t_enc = timed(lambda: enc.push_db(db, raster_out=raster))
        moved = db.numel() * db.element_size() * 2 + raster.numel()
        lines.append(f"  AdaptiveEncoder.push_db alone       {fmt(t_enc)}   reads the dB array twice and writes the raster: "
                     f"{moved / t_enc[0] * 1e-6:.3f} TB/s")
print("\n".join(lines))
