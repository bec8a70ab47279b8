"""Times one lsm_mel_stream_f32 call beside the three batch launches lsm_mel_power_f32 + lsm_power_to_db_f32 +
lsm_spec_to_spikes_f32 on the same number of frames (profiles/mel_stream.txt): 64 streams x 40 filters x 10 hops and
256 x 40 x 100 hops, medians of 21 timed with device events after 5 warm-up rounds, the two alternating, twice.
`--batch-only` times the three batch launches alone and uses nothing newer than them, so that the same file also runs
against an older checkout of the package (`--root DIR`)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
BATCH_ONLY = "--batch-only" in sys.argv
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import _lib, frontend, mel  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
HOP, F, N_FFT = 160, 40, 2048
on, off = frontend.threshold_tables(frontend.SPIKE_THRESHOLDS, 0.1, np.float32)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
h = lambda a: C.c_void_p(a.ctypes.data)
lines = [f"package at {ROOT}, build id {lib.lsm_build_id().decode()}"]


def timed(fn, reps=21, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    # and a batch of calls back to back (the mean hides nothing a single call's event pair adds)
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
    raster = torch.zeros((n, F, H * 4), dtype=torch.uint8, device="cuda")

    # the batch route on H frames per clip: clips of (H - 1) * hop samples have 1 + (H - 1) centred frames
    ms = mel.MelSpectrogram(F, (H - 1) * HOP, H - 1, torch.device("cuda", torch.cuda.current_device()))
    assert ms.hop == HOP and ms.n_frames == H
    clips = audio[:, :(H - 1) * HOP].contiguous()
    power = torch.zeros((n, F, H), dtype=torch.float32, device="cuda")
    bdb = torch.zeros_like(power)
    braster = torch.zeros_like(raster)

    def batch_launches():
        _lib.check(lib.lsm_mel_power_f32(p(clips), n, (H - 1) * HOP, N_FFT, HOP, H, p(ms.window), p(ms.twiddle), p(ms.basis),
                                         p(ms.lo), p(ms.hi), F, p(power), stream))
        _lib.check(lib.lsm_power_to_db_f32(p(power), n, F * H, C.c_float(1e-10), C.c_float(80.0), p(bdb), stream))
        _lib.check(lib.lsm_spec_to_spikes_f32(p(bdb), n, F, H, H, 0, h(on), h(off), 4, 1, p(braster), None, stream))

    if BATCH_ONLY:
        for rep in range(2):
            t = timed(batch_launches)
            lines.append(f"{n} x {F} x {H} frames, pass {rep}: batch power + dB + spikes (3 launches): median {t[0]:.1f} us "
                         f"(min {t[1]:.1f}, max {t[2]:.1f}; back to back {t[3]:.1f} us/round)")
        continue

    nbytes = lib.lsm_mel_stream_state_bytes(F, N_FFT, HOP)
    state = torch.zeros((n, nbytes), dtype=torch.uint8, device="cuda")
    ws = torch.empty((lib.lsm_mel_stream_workspace(n, F, H),), dtype=torch.uint8, device="cuda")
    db = torch.zeros((n, F, H), dtype=torch.float32, device="cuda")
    spow = torch.zeros_like(db)

    def stream_call(db_out=None, power_out=None):
        _lib.check(lib.lsm_mel_stream_f32(p(audio), n, H, N_FFT, HOP, p(ms.window), p(ms.twiddle), p(ms.basis), p(ms.lo),
                                          p(ms.hi), F, None, -40.0, 10.0, h(on), h(off), 4, 1, p(state), p(state), p(raster),
                                          p(power_out), p(db_out), p(ws), int(ws.numel()), stream))

    stream_call()       # state carried in place: from here on every hop of a call completes a frame
    for rep in range(2):
        t_s = timed(stream_call)
        t_d = timed(lambda: stream_call(db, spow))
        t_b = timed(batch_launches)
        for name, t in (("stream (raster only)", t_s), ("stream (raster + dB + power)", t_d),
                        ("batch power + dB + spikes (3 launches)", t_b)):
            lines.append(f"{n} x {F} x {H} frames, pass {rep}: {name}: median {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}; "
                         f"back to back {t[3]:.1f} us/call) = {t[0] * 1e3 / (n * H):.2f} ns per frame")
        lines.append(f"    ratio stream / batch (medians): {t_s[0] / t_b[0]:.3f}; back to back: {t_s[3] / t_b[3]:.3f}")
    torch.cuda.synchronize()
    # the two agree on the frames both made: from a zero state, frame t of the stream is frame t of the clip, up to the
    # clip's last frames, which see its end padding
    state.zero_()
    stream_call(db, spow)
    batch_launches()
    torch.cuda.synchronize()
    both = H - 7
    lines.append(f"    power of the first {both} frames equal bit for bit: "
                 f"{bool(torch.equal(spow[:, :, :both].view(torch.int32), power[:, :, :both].view(torch.int32)))}")

print("\n".join(lines))
