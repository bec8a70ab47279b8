"""Builds the alternative layouts of the reverberation kernel that profiles/reverb.txt compares (exp/reverb_cost.py times
every library it finds under exp/build/): copies of csrc/reverb_body.h with one constant or one index expression replaced,
compiled with csrc/reverb.hip into exp/build/reverb_<name>.so.  The shipped sources carry no switch; a variant that no
longer applies (its text is gone from the header) stops here with an error.  Needs hipcc, no GPU."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lsm_speech_classifier_amd import build  # noqa: E402

CSRC = os.path.join(build.PKG_DIR, "csrc")
OUT = os.path.join(ROOT, "exp", "build")

# name -> [(text in reverb_body.h, its replacement)]
VARIANTS = {
    "r4": [("constexpr int R = 8;", "constexpr int R = 4;")],
    "r16": [("constexpr int R = 8;", "constexpr int R = 16;")],
    "chunk256": [("constexpr int CHUNK = 1024;", "constexpr int CHUNK = 256;")],
    "chunk2048": [("constexpr int CHUNK = 1024;", "constexpr int CHUNK = 2048;")],
    "threads512": [("constexpr int THREADS = 256;", "constexpr int THREADS = 512;")],
    "threads128": [("constexpr int THREADS = 256;", "constexpr int THREADS = 128;")],
    "threads64_chunk512": [("constexpr int THREADS = 256;", "constexpr int THREADS = 64;"),
                           ("constexpr int CHUNK = 1024;", "constexpr int CHUNK = 512;")],
    # the flat layout: sample p at index p, so lanes R samples apart share banks
    "flat": [("lds.samples[(p % R) * STRIDE + p / R]", "lds.samples[p]"),
             ("d[m] = lds.samples[m * STRIDE + row];", "d[m] = lds.samples[row * R + m];")],
}
STUB = """#include <stdarg.h>
#include <stdio.h>
static thread_local char msg[512];
void lsm_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap); }
extern "C" __attribute__((visibility("default"))) const char *lsm_last_error(void) { return msg; }
"""


def main(names):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    body = open(os.path.join(CSRC, "reverb_body.h")).read()
    for name in names:
        work = os.path.join(OUT, "src_" + name)
        os.makedirs(work, exist_ok=True)
        text = body
        for old, new in VARIANTS[name]:
            if text.count(old) != 1:
                raise SystemExit(f"variant {name}: {old!r} occurs {text.count(old)} times in reverb_body.h")
            text = text.replace(old, new)
        with open(os.path.join(work, "reverb_body.h"), "w") as f:
            f.write(text)
        shutil.copy(os.path.join(CSRC, "reverb.hip"), work)
        shutil.copy(os.path.join(CSRC, "lsm_common.h"), work)
        with open(os.path.join(work, "stub.hip"), "w") as f:
            f.write(STUB)
        lib = os.path.join(OUT, f"reverb_{name}.so")
        cmd = [hipcc] + build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "-shared", "-Rpass-analysis=kernel-resource-usage",
                                        os.path.join(work, "reverb.hip"), os.path.join(work, "stub.hip"), "-o", lib]
        report = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        # the batch kernel's lines of the compiler's resource report (the first kernel of the translation unit)
        keep = [line.split("remark:")[-1].split("[-R")[0].strip() for line in report.splitlines()
                if any(k in line for k in (" VGPRs:", "ScratchSize", "Occupancy", "LDS Size"))][:4]
        print(f"{name}: {os.path.relpath(lib, ROOT)}\n    " + " | ".join(keep))


if __name__ == "__main__":
    main(sys.argv[1:] or list(VARIANTS))
