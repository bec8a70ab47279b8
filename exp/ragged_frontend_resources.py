"""Writes the compiler part of profiles/ragged_frontend.txt (`--out`; printed as well).  Needs hipcc, no GPU.

csrc/frontend.hip, csrc/mask.hip and csrc/mel.hip of a checkout of the parent commit (`--parent-tree`) and of this tree, and
csrc/ragged_frontend.hip of this tree, compiled for the device with the build's flags and
`-Rpass-analysis=kernel-resource-usage -S`: every existing kernel's compiler-reported registers, spills, scratch, occupancy
and LDS parent against this tree, its instruction lines likewise (labels renumbered, comments and debug directives dropped),
and the same figures of every new form beside the twin it shares its text with.

`--units frontend,mask,ragged_frontend,step_fused,mel`: the comparison alone, for units that both trees have (the compiler
part of profiles/frontend_launch_request.txt): a kernel symbol that only one tree has, a differing resource report and
differing instruction lines each give a DIFFERS line."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", required=True, help="a checkout of the parent commit")
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--units", default=None, help="comma-separated csrc units that exist in both trees: compare just these, parent "
                                              "against this tree (kernel symbols, resource reports, instruction lines)")
args = ap.parse_args()
UNITS = args.units.split(",") if args.units else ["frontend", "mask", "mel"]
NEW_UNITS = [] if args.units else ["ragged_frontend"]
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def compile_unit(job):
    tree, unit, tmp = job
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(tmp, f"{'parent' if tree != ROOT else 'this'}_{unit}.s")
    p = subprocess.run([hipcc] + build.CFLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S",
                                                 "-Rpass-analysis=kernel-resource-usage",
                                                 os.path.join(tree, "lsm-speech-classifier_amd", "csrc", unit + ".hip"), "-o", out],
                       stderr=subprocess.PIPE, text=True, check=True)
    return out, p.stderr


def remarks(text):
    out, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def bodies(path):
    body, cur, lines_ = {}, None, []
    for raw in open(path):
        s = raw.rstrip("\n")
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", s)
        if m and cur is None:
            cur, lines_ = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", s):
                body[cur], cur = lines_, None
                continue
            t = s.split(";")[0].strip()
            if t and not t.startswith((".p2align", ".loc", ".cfi")):
                lines_.append(re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"\.LBB\d+_", ".LBB_", t)))
    return body


def short(sym):
    s = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip() if shutil.which("c++filt") else sym
    s = s.replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", s.replace("void ", ""))


def row(r):
    return " ".join(f"{r.get(k, '?'):>6s}" for k in FIELDS)


lines = ["hipcc " + " ".join(build.CFLAGS) + " --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/<unit>.hip",
         "columns: " + " | ".join(FIELDS)]
with tempfile.TemporaryDirectory() as tmp:
    jobs = [(args.parent_tree, u, tmp) for u in UNITS] + [(ROOT, u, tmp) for u in UNITS + NEW_UNITS]
    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        done = list(ex.map(compile_unit, jobs))
    res = {(("parent" if t != ROOT else "this"), u): (remarks(err), bodies(out)) for (t, u, _), (out, err) in zip(jobs, done)}
twins = {}
for unit in UNITS:
    (pr, pb), (nr, nb) = res[("parent", unit)], res[("this", unit)]
    same_r = [k for k in pr if nr.get(k) == pr[k]]
    same_b = [k for k in pb if nb.get(k) == pb[k]]
    lines.append(f"csrc/{unit}.hip: {len(pr)} kernels in the parent, {len(nr)} in this tree; resource report identical in every "
                 f"field for {len(same_r)}; instruction lines identical for {len(same_b)} of {len(pb)} functions "
                 f"({sum(len(v) for v in pb.values())} lines compared)")
    for k in pr:
        if k not in same_r or (k in pb and k not in same_b):
            lines.append(f"  DIFFERS: {k}: {pr[k]} -> {nr.get(k)}")
    for k in pb:
        if k not in pr and k not in same_b:
            lines.append(f"  DIFFERS: {k}: instruction lines")
    for k in dict.fromkeys(list(nr) + list(nb)):
        if k not in pr and k not in pb:
            lines.append(f"  DIFFERS: {k}: not in the parent")
    if args.units:
        continue
    if unit == "frontend":
        twins = nr
        for k, r in nr.items():
            if "gammatone_spikes_kernel" in k or "spec_to_spikes_kernel" in k:
                lines.append(f"  {short(k):64s} {row(r)}")
    if unit == "mask":
        for k, r in nr.items():
            lines.append(f"  {short(k):64s} {row(r)}")
rr = res[("this", "ragged_frontend")][0] if NEW_UNITS else {}
if NEW_UNITS:
    lines.append(f"csrc/ragged_frontend.hip: {len(rr)} kernels (new); each beside its twin of csrc/frontend.hip in brackets")
for k, r in rr.items():
    t = k.replace("30gammatone_spikes_ragged_kernel", "23gammatone_spikes_kernel").replace(
        "28spec_to_spikes_ragged_kernel", "21spec_to_spikes_kernel")
    twin = next((v for s, v in twins.items() if s.startswith(t[:t.find("EEv") + 3] if "EEv" in t else t)), None)
    lines.append(f"  {short(k):64s} {row(r)}" + (f"   [{row(twin)}]" if twin and twin is not r else ""))
    if twin and (int(r.get("VGPRs Spill", 0)) > int(twin.get("VGPRs Spill", 0)) or int(r.get("SGPRs Spill", 0)) > int(twin.get("SGPRs Spill", 0))):
        lines.append("    ^ spills its twin does not have")
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
