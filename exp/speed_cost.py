"""Writes profiles/speed_perturb.txt (`--out`; printed as well).  Two parts.

The code object: csrc/speed.hip compiled with the build's flags and `-save-temps` into a temporary directory, and
`speed_kernel`'s metadata read from the assembly -- VGPRs, SGPRs, static LDS, scratch, spills.  Needs hipcc, no GPU
(`--no-timing` stops here).

The cost: 256 one-second clips with the factors 0.9 / 1.0 / 1.1 drawn uniformly (`frontend.speed_plan`), played in one
`lsm_speed_f32` launch, beside what the library offered for the same job before: the clips of each non-unit factor gathered
with `index_select`, resampled by `frontend.Resampler(14400)` and `frontend.Resampler(17600)` into buffers of their own, and
put back with `index_copy_` (the unperturbed clips stay where they are).  Both timed with device events in the same
process, alternating, medians of 20 after 4 warm-up runs, `--rounds` times over so that the spread between equal runs
stands beside the figures; the two outputs are compared byte for byte, and two clips with the NumPy restatement.  The
fused gammatone front-end launch for 256 clips x 128 filters is timed in the same rounds for scale."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-timing", action="store_true", help="the code object only (no GPU needed)")
args = ap.parse_args()

lines = []


def code_object():
    """speed_kernel's resource figures out of the assembly's metadata."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([hipcc] + build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "-save-temps", "-c",
                                                        os.path.join(build.PKG_DIR, "csrc", "speed.hip"), "-o", "speed.o"], cwd=tmp)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        text = open(os.path.join(tmp, asm[0])).read()
    meta = text[text.index("amdhsa.kernels"):]
    entry = next(block for block in meta.split("  - .agpr_count") if "speed_kernel" in block)

    def field(name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, entry).group(1))
    lines.append("speed_kernel's code object (hipcc " + " ".join(build.CFLAGS) + ", metadata of the assembly):")
    lines.append(f"  VGPRs {field('vgpr_count')}, SGPRs {field('sgpr_count')}, static LDS {field('group_segment_fixed_size')} bytes "
                 f"(dynamic: the bank's largest table), scratch {field('private_segment_fixed_size')} bytes, "
                 f"VGPR spills {field('vgpr_spill_count')}, SGPR spills {field('sgpr_spill_count')}, "
                 f"kernel arguments {field('kernarg_segment_size')} bytes")
    scratch = len(re.findall(r"^\s*scratch_(?:load|store)", text, re.M))
    # the chosen design's first four numbers: one load from the kernel arguments at a scalar offset (the table starts at 0x30)
    scalar = re.search(r"s_load_dwordx4 s\[\d+:\d+\], s\[\d+:\d+\], 0x30", text) is not None
    lines.append(f"  scratch instructions in the assembly: {scratch}; the design table is read from the kernel arguments with "
                 f"scalar loads at a scalar offset: {'yes' if scalar else 'not found'}")
    assert field("private_segment_fixed_size") == 0 and scratch == 0, "speed_kernel uses scratch"


code_object()

if not args.no_timing:
    import torch
    import speed_restatement as SR
    from lsm_speech_classifier_amd import _lib, frontend, synth

    lib = _lib.load()
    _lib.require_gpu()
    lines += [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}"]
    B, N = 256, 16000
    FACTORS = ["0.9", "1.0", "1.1"]

    def timed(fn, reps=20, warm=4):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def void(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    audio_h = synth.white_noise(B, seed=5)
    audio = torch.from_numpy(audio_h).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    sp = frontend.SpeedPerturber(FACTORS)
    choice = frontend.speed_plan(B, len(FACTORS), seed=3).choice
    rows_h = sp.rows_of(choice, B)
    rows = torch.from_numpy(rows_h).cuda()
    lines.append(f"{B} clips x {N} samples, factors {FACTORS}: {[int((choice == k).sum()) for k in range(3)]} clips each; "
                 f"dynamic LDS of the launch {sp.lds_bytes} bytes")
    out_one = torch.empty_like(audio)

    def one_launch():
        rc = lib.lsm_speed_f32(void(audio), 0, B, N, void(sp.taps_dev), sp.n_taps_total, C.c_void_p(sp.designs.ctypes.data),
                               len(sp.designs), void(rows), N, void(out_one), stream)
        assert rc == 0, lib.lsm_last_error()

    groups = []
    for k, rate in ((0, 14400), (2, 17600)):
        idx = torch.from_numpy(np.flatnonzero(choice == k)).cuda()
        groups.append((idx, frontend.Resampler(rate), torch.empty((len(idx), N), dtype=torch.float32, device="cuda")))
    out_grouped = audio.clone()                  # the unperturbed clips are where they belong already

    def grouped():
        for idx, rs, buf in groups:
            rs.resample(audio.index_select(0, idx), n_out=N, out=buf)
            out_grouped.index_copy_(0, idx, buf)

    def resample_only():
        for idx, rs, buf in groups:
            rs.resample(buf, n_out=N, out=out_grouped[:len(idx)])

    fe = frontend.SpikeFrontEnd(128, "gammatone")
    fe.encode(audio)
    one, old = [], []
    for rnd in range(1, args.rounds + 1):
        t = timed(one_launch)
        one.append(t[0])
        lines.append(f"  round {rnd}: one lsm_speed_f32 launch                          median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
        t = timed(grouped)
        old.append(t[0])
        lines.append(f"  round {rnd}: grouped: 2 x (index_select, Resampler.resample, index_copy_) median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
        t = timed(lambda: fe.encode(audio))
        lines.append(f"  round {rnd}: front end, 256 clips x 128 gammatone filters       median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
    t = timed(resample_only)
    lines.append(f"  the grouped path's two Resampler.resample launches alone (no gather, no scatter): median {t[0]:.1f} us "
                 f"(min {t[1]:.1f}, max {t[2]:.1f})")
    one_launch()
    out_grouped.copy_(audio)
    grouped()
    torch.cuda.synchronize()
    got = out_one.cpu().numpy()
    lines.append(f"  the one launch equals the grouped path byte for byte: {got.tobytes() == out_grouped.cpu().numpy().tobytes()}")
    picks = [int(np.flatnonzero(choice == 0)[0]), int(np.flatnonzero(choice == 2)[0])]
    want = SR.perturb_batch(audio_h[picks], sp.tables, rows_h[picks], N)
    lines.append(f"  clips {picks} of the timed batch equal the restatement byte for byte: {got[picks].tobytes() == want.tobytes()}")
    spread = max(max(one) - min(one), max(old) - min(old))
    m_one, m_old = float(np.median(one)), float(np.median(old))
    lines.append(f"  medians over the rounds: one launch {m_one:.1f} us, grouped path {m_old:.1f} us; spread between equal rounds "
                 f"up to {spread:.1f} us")
    lines.append("  the one launch takes " + ("no longer than the grouped path" if m_one <= m_old + spread else
                                              "LONGER than the grouped path beyond the spread") + f" ({m_one / m_old:.2f} x)")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
