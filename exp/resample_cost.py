"""Times the device resampler (profiles/resample.txt): one `lsm_resample_f32` launch on 256 one-second clips at 48000 and at
44100 Hz, float32 and int16, and one `lsm_resample_stream_f32` call on 64 streams x 10 units, medians of 20 launches timed
with device events after 5 warm-ups; beside them what the parent commit does with the same 256 clips,
`scipy.signal.resample_poly` clip by clip in this process (`create_dataset.load_audio_file`'s route), by the wall clock."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import _lib, frontend  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
lines = [f"package at {ROOT}, build id {lib.lsm_build_id().decode()}"]


def timed(fn, reps=20, warm=5):
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


N_CLIPS, N_STREAMS, UNITS = 256, 64, 10
for rate in (48000, 44100):
    rng = np.random.default_rng(rate)
    host = (rng.standard_normal((N_CLIPS, rate)) * 0.1).astype(np.float32)
    rs = frontend.Resampler(rate)
    out = torch.empty((N_CLIPS, 16000), dtype=torch.float32, device="cuda")
    for name, clips in (("float32", torch.from_numpy(host).cuda()),
                        ("int16", torch.from_numpy(np.round(host * 32767).astype(np.int16)).cuda())):
        t = timed(lambda: rs.resample(clips, n_out=16000, out=out))
        moved = clips.numel() * clips.element_size() + out.numel() * 4
        lines.append(f"{rate} Hz, {N_CLIPS} clips of 1 s, {name}: lsm_resample_f32 median {t[0]:.1f} us (min {t[1]:.1f}, max "
                     f"{t[2]:.1f}; back to back {t[3]:.1f} us/launch) = {N_CLIPS / t[0]:.2f} M clips/s, "
                     f"{moved / t[0] * 1e-6:.2f} TB/s of input read once and output written")
    st = frontend.ResampleStream(rate, N_STREAMS)
    pcm = torch.from_numpy(np.round(host[:N_STREAMS, :UNITS * st.unit_in] * 32767).astype(np.int16)).cuda()
    sout = torch.empty((N_STREAMS, UNITS * st.unit_blocks * st.up), dtype=torch.float32, device="cuda")
    t = timed(lambda: st.push(pcm, out=sout))
    lines.append(f"{rate} Hz, {N_STREAMS} streams x {UNITS} units of {st.unit_in} samples, int16: lsm_resample_stream_f32 "
                 f"(two kernels) median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}; back to back {t[3]:.1f} us/call)")
    # the parent commit's route: one clip at a time on one core
    from scipy.signal import resample_poly
    resample_poly(host[0], rs.up, rs.down)
    t0 = time.perf_counter()
    ref = np.stack([resample_poly(x, rs.up, rs.down).astype(np.float32) for x in host])
    dt = time.perf_counter() - t0
    got = rs.resample(host, n_out=16000).cpu().numpy()
    lines.append(f"{rate} Hz, {N_CLIPS} clips of 1 s, float32: scipy.signal.resample_poly, one process: {dt * 1e3:.1f} ms "
                 f"({dt / N_CLIPS * 1e6:.0f} us per clip); max |device - host| = {np.abs(got - ref).max():.2e}")
print("\n".join(lines))
