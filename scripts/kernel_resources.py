#!/usr/bin/env python3
"""Register, scratch and occupancy figures of the library's kernels, from the compiler alone (no GPU needed).

Compiles HIP sources of mrla_amd/csrc for the device only with -Rpass-analysis=kernel-resource-usage (the product
build's flags, including the Makefile's per-file -fno-slp-vectorize exceptions) and prints one line per kernel:
name, VGPRs, AGPRs, scratch bytes per lane, waves per SIMD, static LDS bytes.  A kernel with scratch spills registers
inside its loops; one whose waves / SIMD fall short of what its planner assumes runs fewer workgroups per CU than planned.
Nothing of the product build is replaced: objects go to a temporary directory.

    python scripts/kernel_resources.py                 # every source of the library
    python scripts/kernel_resources.py conv1x1.hip     # one file
    python scripts/kernel_resources.py --scratch-only  # only the kernels that spill
"""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mrla_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-function"]           # Makefile: FLAGS
NO_SLP = {"light_nhwc_bwd.hip", "light_nhwc_wide.hip", "light_nhwc_lean.hip", "tokens_nhwc.hip"}   # Makefile: FLAGS +=
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves",
          "LDS Size [bytes/block]": "lds"}
_REMARK = re.compile(r"remark:\s+(.+?):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def find_hipcc():
    cand = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    return cand if os.path.exists(cand) else shutil.which("hipcc")


def demangle(names):
    """Readable names where a demangler is at hand; binutils' c++filt garbles the bf16 / fp16 template arguments
    (DF16b, DF16_) of older releases: such names stay mangled."""
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (TypeError, OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    return {n: (n if "_Accum" in o or not o else o) for n, o in zip(names, out)}


def parse_remarks(text):
    """[{mangled, vgprs, agprs, scratch, waves, lds}] from the compiler's remark stream (one block per kernel)."""
    kernels, cur = [], None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"mangled": val}
            kernels.append(cur)
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return kernels


def kernel_resources(source, arch="gfx950", hipcc=None, csrc=CSRC):
    """Compile one source of mrla_amd/csrc (of this checkout, or `csrc` of another) for the device and return its kernels'
    figures, names demangled."""
    hipcc = hipcc or find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found (set HIPCC)")
    flags = FLAGS + (["-fno-slp-vectorize"] if os.path.basename(source) in NO_SLP else [])
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *flags, f"--offload-arch={arch}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.basename(source), "-o", os.path.join(tmp, "device.o")]
        run = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if run.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{run.stderr[-4000:]}")
    kernels = parse_remarks(run.stderr)
    names = demangle([k["mangled"] for k in kernels])
    for k in kernels:
        k["name"] = names[k["mangled"]]
        k["file"] = os.path.basename(source)
    return kernels


def short(name):
    """`void mrla::kernel<args>(params)` -> `kernel<args>`."""
    name = re.sub(r"^void\s+", "", name)
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            name = name[:i]
            break
    return name.replace("mrla::", "").replace("(anonymous namespace)::", "")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", help="files of mrla_amd/csrc (default: all *.hip)")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--scratch-only", action="store_true", help="print only the kernels with scratch")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    sources = a.sources or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        per_file = list(pool.map(lambda s: kernel_resources(s, a.arch), sources))
    print(f"{'file':24s} {'VGPR':>4s} {'AGPR':>4s} {'scratch':>7s} {'waves':>5s} {'LDS':>6s}  kernel")
    spilled = 0
    for kernels in per_file:
        for k in kernels:
            spilled += k["scratch"] > 0
            if a.scratch_only and not k["scratch"]:
                continue
            print(f"{k['file']:24s} {k['vgprs']:4d} {k['agprs']:4d} {k['scratch']:7d} {k['waves']:5d} {k['lds']:6d}  {short(k['name'])}")
    print(f"# {sum(map(len, per_file))} kernels, {spilled} with scratch", file=sys.stderr)


if __name__ == "__main__":
    main()
