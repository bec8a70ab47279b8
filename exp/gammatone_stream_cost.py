"""Times one lsm_gammatone_stream_f64 launch beside one lsm_gammatone_spec_f64 launch of the same sample-channels
(profiles/gammatone_stream.txt): 64 streams x 128 filters x 10 hops and 256 x 128 x 100 hops, medians of 21 launches timed
with device events after 5 warm-up launches, the two kernels alternating, twice."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import _lib, frontend  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
HOP, NWIN, F = 160, 400, 128
tab = frontend.gammatone_filter_table(16000, F, 50)
flags = frontend.coef_flags(tab)
coefs = torch.from_numpy(tab).cuda()
on, off = frontend.threshold_tables(frontend.SPIKE_THRESHOLDS, 0.1, np.float64)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
lines = []


def timed(fn, reps=21, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    # and a batch of launches back to back (the mean hides nothing a single launch's event pair adds)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), a.elapsed_time(b) * 1e3 / reps


for n, H in ((64, 10), (256, 100)):
    g = torch.Generator(device="cpu").manual_seed(1)
    audio = (torch.randn((n, H * HOP), generator=g) * 0.1).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = lib.lsm_gammatone_stream_state_bytes(F, NWIN, HOP)
    state = torch.zeros((n, nbytes), dtype=torch.uint8, device="cuda")
    raster = torch.zeros((n, F, H * 4), dtype=torch.uint8, device="cuda")
    db = torch.zeros((n, F, H), dtype=torch.float64, device="cuda")

    def stream_launch(db_out=None):
        _lib.check(lib.lsm_gammatone_stream_f64(p(audio), n, H, p(coefs), F, NWIN, HOP, None, -70.0, -20.0,
                                                C.c_void_p(on.ctypes.data), C.c_void_p(off.ctypes.data), 4, 1, p(state), p(state),
                                                p(raster), None, p(db_out), flags, stream))

    ncols = (H * HOP - NWIN) // HOP + 1
    sdb = torch.zeros((n, F, ncols), dtype=torch.float64, device="cuda")

    def spec_launch():
        _lib.check(lib.lsm_gammatone_spec_f64(p(audio), n, H * HOP, p(coefs), F, NWIN, HOP, ncols, None, p(sdb), flags, stream))

    # alternate the two, twice
    for rep in range(2):
        t_s = timed(stream_launch)
        t_d = timed(lambda: stream_launch(db))
        t_y = timed(spec_launch)
        sc = n * H * HOP * F
        for name, t in (("stream (raster only)", t_s), ("stream (raster + dB)", t_d), ("split lsm_gammatone_spec_f64 (dB)", t_y)):
            lines.append(f"{n} x {F} x {H} hops, pass {rep}: {name}: median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}; "
                         f"back to back {t[3]:.1f} us/launch) = {t[0] * 1e3 / sc * 1e3:.3f} ps per sample-channel")
        lines.append(f"    ratio stream / split (medians): {t_s[0] / t_y[0]:.3f}; back to back: {t_s[3] / t_y[3]:.3f}")
    torch.cuda.synchronize()
    # the two agree on the columns both made (stream from zero state: column c is the split kernel's column c)
    state.zero_()
    stream_launch(db)
    spec_launch()
    torch.cuda.synchronize()
    lines.append(f"    dB columns equal bit for bit: {bool(torch.equal(db[:, :, :ncols], sdb))}")

print("\n".join(lines))
