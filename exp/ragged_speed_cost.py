"""Writes profiles/ragged_speed.txt's measured lines (`--out`; printed as well).  Two parts.

The code objects: csrc/speed.hip compiled with the build's flags and the compiler's own resource report
(`-Rpass-analysis=kernel-resource-usage`) for both instantiations of `speed_kernel` -- the plain one behind `lsm_speed_f32`
and the ragged one behind `lsm_speed_ragged_f32`.  With `--parent-csrc DIR` (the csrc/ of the parent commit, its include/
beside it) the parent's `speed_kernel` is compiled the same way, the plain instantiation's line must equal it and the two
kernels' instructions are compared one for one; the ragged one must use no scratch.  Needs hipcc, no GPU (`--no-timing`
stops here; `--no-code` skips it).

The cost: 256 one-second clips with the factors 0.9 / 1.0 / 1.1 drawn uniformly (`frontend.speed_plan`), device events,
every figure the median of 50 launches after 5 warm-up launches, the forms ALTERNATING within a round and every round starting
one form further on (so that no form always follows the same one), `--rounds` (5) rounds; per form the median of the rounds'
medians and their range.
  (a) `lsm_speed_f32` of the parent build's library (`--parent-lib`, loaded beside this one) and of this tree: each median must
      lie inside the other's range over the rounds, the kernel being meant to be unchanged.  `--copy-beside` times this tree's
      library a second time, from a copy of the file loaded beside the first as the parent's is: the same code in the
      parent's place.
  (b) `lsm_speed_ragged_f32` at full lengths in the same rounds; the same launch with lengths of 0.3 to 1.0 s (whole bins of
      160 samples, uniform); and what served such clips before: the clips grouped by length, per group an `index_select`, a
      cut to the group's length and one `lsm_speed_f32` launch at n_in = that length (no scatter back is counted).
The outputs are compared byte for byte: the two builds' `lsm_speed_f32`, the ragged launch against it up to every clip's n', and
against the grouped launches."""
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
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-timing", action="store_true", help="the code objects only (no GPU needed)")
ap.add_argument("--no-code", action="store_true", help="the launches only")
ap.add_argument("--parent-csrc", default=None, help="csrc/ of the parent commit: compare speed_kernel's resource report")
ap.add_argument("--copy-beside", action="store_true",
                help="time lsm_speed_f32 of a copy of this tree's library too, loaded beside the first as the parent's is")
ap.add_argument("--parent-lib", default=None, help="liblsm_hip.so of the parent commit: time its lsm_speed_f32 beside this build's")
args = ap.parse_args()

lines = []
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def instructions(asm, key):
    """The instructions of the kernel whose mangled name holds ``key``, out of the assembly: no comments, no directives, the
    block labels' function number dropped."""
    m = re.search(r"^_ZN[^\n]*%s[^\n]*:[^\n]*\n(.*?)\.Lfunc_end" % key, asm, re.S | re.M)
    body = [line.split(";")[0].rstrip() for line in m.group(1).splitlines()]
    return [re.sub(r"\.LBB\d+_", ".LBB_", line) for line in body if line.strip() and not line.strip().startswith(".")]


def reports(csrc, include):
    """({kernel's mangled name: {field: value}} of speed.hip under ``csrc``, from the compiler's resource remarks; the
    assembly)."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([hipcc] + build.CFLAGS + ["-I", include, "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj",
                                                       "-c", os.path.join(csrc, "speed.hip"), "-o", os.path.join(tmp, "speed.o")],
                             capture_output=True, text=True, check=True).stderr
        asm = open(os.path.join(tmp, next(f for f in os.listdir(tmp) if f.endswith("gfx950.s")))).read()
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for f in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(f) + r": (\d+)", line)
            if m and name:
                out[name][f] = int(m.group(1))
    return out, asm


def report_line(r):
    return ", ".join(f"{f} {r[f]}" for f in FIELDS)


def code_objects():
    ours, asm = reports(os.path.join(build.PKG_DIR, "csrc"), os.path.join(ROOT, "include"))
    plain = next(v for k, v in ours.items() if "speed_kernelILb0" in k)
    ragged = next(v for k, v in ours.items() if "speed_kernelILb1" in k)
    lines.append("speed.hip's code objects (hipcc " + " ".join(build.CFLAGS) + ", the compiler's resource report; dynamic LDS is the "
                 "bank's largest table):")
    lines.append(f"  speed_kernel<false> (lsm_speed_f32):        {report_line(plain)}")
    lines.append(f"  speed_kernel<true>  (lsm_speed_ragged_f32): {report_line(ragged)}")
    assert plain["ScratchSize [bytes/lane]"] == 0 and ragged["ScratchSize [bytes/lane]"] == 0, "a speed kernel uses scratch"
    if args.parent_csrc:
        inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(args.parent_csrc))), "include")
        theirs, parent_asm = reports(args.parent_csrc, inc)
        assert len(theirs) == 1, sorted(theirs)
        parent = next(iter(theirs.values()))
        lines.append(f"  the parent's speed_kernel:                  {report_line(parent)}")
        lines.append("  lsm_speed_f32's kernel has the parent's report, field for field: " + ("yes" if parent == plain else "NO"))
        assert parent == plain, "lsm_speed_f32's kernel compiles to other resources than in the parent"
        mine, before = instructions(asm, "speed_kernelILb0"), instructions(parent_asm, "speed_kernelE")
        lines.append(f"  its {len(mine)} instructions are the parent's {len(before)}, one for one: " + ("yes" if mine == before else "NO"))


if not args.no_code:
    code_objects()

if not args.no_timing:
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, synth

    lib = _lib.load()
    _lib.require_gpu()
    lines += [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}"]
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.lsm_build_id.restype = C.c_char_p
        parent.lsm_speed_f32.restype = C.c_int
        parent.lsm_speed_f32.argtypes = _lib.SPEED_SIGS["lsm_speed_f32"][1]
        lines.append(f"parent library: build id {parent.lsm_build_id().decode()}")
    copy = None
    if args.copy_beside:
        # this tree's own library once more, from a copy of the file: loaded beside the first like the parent's, same code
        import shutil
        tmp_lib = os.path.join(tempfile.mkdtemp(), "liblsm_hip_copy.so")
        shutil.copy(build.lib_path(), tmp_lib)
        copy = C.CDLL(tmp_lib)
        copy.lsm_speed_f32.restype = C.c_int
        copy.lsm_speed_f32.argtypes = _lib.SPEED_SIGS["lsm_speed_f32"][1]
    B, N, HOP = 256, 16000, 160
    FACTORS = ["0.9", "1.0", "1.1"]

    def timed(fn, reps=50, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    def void(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    audio_h = synth.white_noise(B, seed=5)
    audio = torch.from_numpy(audio_h).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    sp = frontend.SpeedPerturber(FACTORS)
    choice = frontend.speed_plan(B, len(FACTORS), seed=3).choice
    rows_h = sp.rows_of(choice, B)
    rows = torch.from_numpy(rows_h).cuda()
    designs = C.c_void_p(sp.designs.ctypes.data)
    bins_h = np.random.RandomState(7).randint(48, 101, size=B)                      # 0.3 to 1.0 s in whole bins
    full = torch.full((B,), N, dtype=torch.int32, device="cuda")
    short_h = (bins_h * HOP).astype(np.int32)
    short = torch.from_numpy(short_h).cuda()
    lines.append(f"{B} clips x {N} samples, factors {FACTORS}: {[int((choice == k).sum()) for k in range(3)]} clips each; dynamic LDS "
                 f"of a launch {sp.lds_bytes} bytes; ragged lengths {int(short_h.min())} .. {int(short_h.max())} samples, mean "
                 f"{short_h.mean() / N:.3f} of the row, {len(set(bins_h.tolist()))} distinct")
    outs = {k: torch.empty_like(audio) for k in ("this", "parent", "copy", "ragged", "short")}
    counts = [torch.empty((B,), dtype=torch.int32, device="cuda") for _ in range(2)]

    def twin(which, out):
        def run():
            rc = which.lsm_speed_f32(void(audio), 0, B, N, void(sp.taps_dev), sp.n_taps_total, designs, len(sp.designs), void(rows),
                                     N, void(out), stream)
            assert rc == 0, lib.lsm_last_error()
        return run

    def ragged(lengths, out):
        def run():
            rc = lib.lsm_speed_ragged_f32(void(audio), 0, B, N, void(lengths), void(sp.taps_dev), sp.n_taps_total, designs,
                                          len(sp.designs), void(rows), N, void(out), void(counts[0]), void(counts[1]), N // HOP,
                                          stream)
            assert rc == 0, lib.lsm_last_error()
        return run

    groups = []
    for n in sorted(set(short_h.tolist())):
        idx_h = np.flatnonzero(short_h == n)
        n_out = min(-(-n * 10 // 9), N)                              # the longest n' of a group: its clips at 9/10
        groups.append((n, torch.from_numpy(idx_h).cuda(), idx_h, n_out,
                       torch.empty((len(idx_h), n_out), dtype=torch.float32, device="cuda")))

    def grouped():
        for n, idx, _, n_out, buf in groups:
            x = audio.index_select(0, idx)[:, :n].contiguous()
            rc = lib.lsm_speed_f32(void(x), 0, len(idx), n, void(sp.taps_dev), sp.n_taps_total, designs, len(sp.designs),
                                   void(rows.index_select(0, idx)), n_out, void(buf), stream)
            assert rc == 0, lib.lsm_last_error()

    forms = ([("lsm_speed_f32, parent build", twin(parent, outs["parent"]))] if parent is not None else []) + [
        ("lsm_speed_f32, this tree", twin(lib, outs["this"]))] + (
        [("lsm_speed_f32, this tree, a copy loaded beside", twin(copy, outs["copy"]))] if copy is not None else []) + [
        ("lsm_speed_ragged_f32, full lengths", ragged(full, outs["ragged"])),
        ("lsm_speed_ragged_f32, 0.3 to 1.0 s", ragged(short, outs["short"])),
        (f"grouped by length: {len(groups)} x (index_select, cut, lsm_speed_f32)", grouped)]
    medians = {name: [] for name, _ in forms}
    for rnd in range(1, args.rounds + 1):
        turn = forms[(rnd - 1) % len(forms):] + forms[:(rnd - 1) % len(forms)]     # alternating: every form once per round, and
        for name, fn in turn:                                        # each round starts one form further on
            medians[name].append(timed(fn, reps=50 if fn is not grouped else 10))
        lines.append(f"  round {rnd} (from form {(rnd - 1) % len(forms) + 1} on): " + "; ".join(f"{medians[name][-1]:.1f}" for name, _ in forms)
                     + " us")
    width = max(len(name) for name, _ in forms)
    for name, _ in forms:
        m = medians[name]
        lines.append(f"  {name:<{width}}  median of {len(m)} rounds {np.median(m):8.1f} us (rounds {min(m):.1f} to {max(m):.1f})")
    if parent is not None:
        p, t = medians["lsm_speed_f32, parent build"], medians["lsm_speed_f32, this tree"]
        inside = min(t) <= np.median(p) <= max(t) and min(p) <= np.median(t) <= max(p)
        lines.append(f"  (a) each build's median lies inside the other's range over the rounds: {'yes' if inside else 'NO'} "
                     f"(this tree / parent = {np.median(t) / np.median(p):.3f})")
    t, r, s = (float(np.median(medians[k])) for k in ("lsm_speed_f32, this tree", "lsm_speed_ragged_f32, full lengths",
                                                      "lsm_speed_ragged_f32, 0.3 to 1.0 s"))
    g = float(np.median(medians[forms[-1][0]]))
    lines.append(f"  (b) ragged at full lengths / lsm_speed_f32 = {r / t:.3f}; ragged at 0.3 to 1.0 s / ragged at full lengths = "
                 f"{s / r:.3f}; grouped by length / ragged at 0.3 to 1.0 s = {g / s:.2f}")
    # the bytes
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    this = outs["this"].cpu().numpy()
    if parent is not None:
        lines.append(f"  lsm_speed_f32 of the two builds gives the same bytes: {this.tobytes() == outs['parent'].cpu().numpy().tobytes()}")
    new_full = frontend.speed_ragged_lengths(np.full(B, N), choice, sp, N)
    got = outs["ragged"].cpu().numpy()
    same = all(got[b, :new_full[b]].tobytes() == this[b, :new_full[b]].tobytes() and not got[b, new_full[b]:].any() for b in range(B))
    lines.append(f"  the ragged launch at full lengths equals lsm_speed_f32 up to every clip's n' and is +0.0 behind: {same}")
    new_short = frontend.speed_ragged_lengths(short_h, choice, sp, N)
    got = outs["short"].cpu().numpy()
    same = counts[0].cpu().numpy().tolist() == new_short.tolist()
    for n, _, idx_h, n_out, buf in groups:
        alone = buf.cpu().numpy()
        same = same and all(got[b, :new_short[b]].tobytes() == alone[k, :new_short[b]].tobytes() and not got[b, new_short[b]:].any()
                            for k, b in enumerate(idx_h))
    lines.append(f"  the ragged launch at 0.3 to 1.0 s equals the grouped launches up to every clip's n', is +0.0 behind, and its "
                 f"counts are the host formula's: {same}")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
