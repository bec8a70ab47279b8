"""Times the noise mixer (profiles/noise_mix.txt): `lsm_mix_f32` on 256 one-second clips with banks of 16 000 and 960 000
samples per row, `lsm_mix_stream_f32` on 256 streams x 1600 samples, `NoiseMixer.mix` with its parameter uploads, the NumPy
restatement of the same batch on the host, and -- the yardstick -- the fused gammatone front-end launch for 256 clips x 128
filters, which this mixer is put in front of.  Medians of 40 calls timed with device events after 8 warm-up calls, twice,
alternating, so that the spread between equal runs stands beside the figures.  The timed batch is also compared with the
restatement byte for byte."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mix_restatement as M  # noqa: E402
from lsm_speech_classifier_amd import _lib, frontend, synth  # noqa: E402

lib = _lib.load()
_lib.require_gpu()
lines = [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}"]


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
    return f"median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f}; back to back {t[3]:.1f} us/call)"


def void(t):
    return C.c_void_p(t.data_ptr())


B, N, ROWS = 256, 16000, 6
audio_h = synth.white_noise(B, seed=5)
audio = torch.from_numpy(audio_h).cuda()
out = torch.empty_like(audio)
plan = frontend.mix_plan(B, ROWS, 16000, (0.0, 20.0), max_shift=1600, level_db=(-6.0, 0.0), seed=3)
stream = torch.cuda.current_stream().cuda_stream
mixers = {}
for L in (16000, 960000):
    bank = (np.random.default_rng(L).standard_normal((ROWS, L)) * 0.05).astype(np.float32)
    mixers[L] = (bank, frontend.NoiseMixer(bank))
dev = dict(rows=torch.from_numpy(plan.rows).cuda(), shift=torch.from_numpy(plan.shift).cuda(),
           scale=torch.from_numpy(plan.scale).cuda(), ratio=torch.from_numpy(frontend.snr_ratio(plan.snr_db, B)).cuda())


def launch(L, offsets):
    mixer = mixers[L][1]
    _lib.check(lib.lsm_mix_f32(void(audio), B, N, void(mixer.noise), ROWS, L, void(dev["rows"]), void(offsets),
                               void(dev["shift"]), void(dev["scale"]), void(dev["ratio"]), void(out), None, None, stream))


fe = frontend.SpikeFrontEnd(128, "gammatone")
raster = fe.encode(audio)
ms = frontend.MixStream(mixers[16000][1], B)
ms.set(np.arange(B), plan.snr_db, 0.01, plan.rows, plan.scale)
push = audio[:, :1600].contiguous()
push_out = torch.empty_like(push)
for rnd in (1, 2):
    for L in (16000, 960000):
        offsets = torch.from_numpy((plan.offsets.astype(np.int64) * (L // 16000)).astype(np.int32)).cuda()
        t = timed(lambda: launch(L, offsets))
        moved = 3 * audio.numel() * 4 + 2 * audio.numel() * 4           # clip read twice, noise twice, out once
        lines.append(f"  round {rnd}: lsm_mix_f32 256 x 16000, bank {ROWS} x {L:6d}   {fmt(t)}   "
                     f"{moved / t[0] * 1e-6:.2f} TB/s counting both reads of clip and noise")
    t = timed(lambda: mixers[16000][1].mix(audio, plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale, out=out))
    lines.append(f"  round {rnd}: NoiseMixer.mix (5 small uploads + launch)        {fmt(t)}")
    t = timed(lambda: ms.push(push, out=push_out))
    lines.append(f"  round {rnd}: MixStream.push 256 x 1600                        {fmt(t)}")
    t = timed(lambda: fe.encode(audio))
    lines.append(f"  round {rnd}: front end, 256 clips x 128 gammatone filters     {fmt(t)}")

# correctness at the timed size, and the host's time for the same batch
bank, mixer = mixers[16000]
t0 = time.perf_counter()
want, _, _ = M.mix(audio_h, bank, frontend.snr_ratio(plan.snr_db, B), plan.rows, plan.offsets, plan.shift, plan.scale)
t_rest = time.perf_counter() - t0
got = mixer.mix(audio, plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale).cpu().numpy()
lines.append(f"  the timed batch equals the restatement byte for byte: {got.tobytes() == want.tobytes()}")


def naive():
    """What a host recipe does: np.roll, two np.sum reductions and a scaled add per clip."""
    y = np.empty_like(audio_h)
    for b in range(B):
        x = np.roll(audio_h[b], plan.shift[b]).astype(np.float64) * plan.scale[b]
        v = np.resize(np.roll(bank[plan.rows[b]], -int(plan.offsets[b])), N).astype(np.float64)
        g = np.sqrt(np.sum(x * x) * 10.0 ** (-plan.snr_db[b] / 10.0) / np.sum(v * v))
        y[b] = (x + g * v).astype(np.float32)
    return y


ts = []
for _ in range(5):
    t0 = time.perf_counter()
    naive()
    ts.append(time.perf_counter() - t0)
lines.append(f"  host, one core: the vectorised restatement {t_rest * 1e3:.1f} ms per batch; a plain NumPy recipe "
             f"{np.median(ts) * 1e3:.1f} ms per batch = {np.median(ts) / B * 1e6:.1f} us per clip (median of 5)")
print("\n".join(lines))
