#!/usr/bin/env python3
"""Do two trees compile the same kernels?  The gate for changes that share code between kernels (no GPU needed).

Compiles the named sources of mrla_amd/csrc of two checkouts for the device only (the product build's flags, including the
Makefile's per-file exceptions, as scripts/kernel_resources.py has them) to assembly, cuts the assembly per kernel (a
function's opening directives, its code, its .amdhsa_kernel descriptor and the symbols set behind that), normalises what
may differ without the code differing -- the kernel's own symbol, the numbering of local labels, the anonymous-namespace
prefix, comments and debug lines -- and compares whole instruction streams, kernel descriptors included.  It looks for no
particular instruction.  Prints the kernels that differ or exist on one side only, and for every kernel both trees' VGPR, AGPR,
SGPR, scratch, LDS and occupancy figures (from scripts/kernel_resources.py).  Exit status 1 if anything differs.

    python scripts/kernel_isa_diff.py /path/to/parent/checkout conv1x1.hip conv1x1_wide.hip
    python scripts/kernel_isa_diff.py /path/to/parent/checkout          # the five conv1x1 sources
    python scripts/kernel_isa_diff.py /path/to/parent/checkout --all    # every source of the Makefile's SRC list

A kernel that lost a template argument has another mangled name than the instance it came from: --map 'REGEX=REPL'
(repeatable, re.sub on the PARENT's mangled names before the kernels are paired) names the pairing, e.g.
--map 'Lb0EEEvPKT_=EEvPKT_' for a trailing `false` in front of a (const T*, ...) parameter list.  Two parent kernels that
map to one name are an error.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

import kernel_resources as kr

CONV1X1 = ["conv1x1.hip", "conv1x1_wide.hip", "conv1x1_kstream.hip", "conv1x1_wgrad.hip", "conv1x1_f32.hip"]
FIGURES = ("vgprs", "agprs", "sgprs", "scratch", "lds", "waves")
_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
_FUNCTION = re.compile(r"\s*\.type\s+(\S+),@function")
_OPENING = re.compile(r"\s*\.(section|text|globl|weak|protected|hidden|p2align)\b")
_DEBUG = re.compile(r"\s*\.(loc|file|cfi_\w+|ident|addrsig\w*|section\s+\.debug\w*)\b")


def csrc_of(tree):
    return os.path.join(os.path.abspath(tree), "mrla_amd", "csrc")


def assembly(csrc, source, arch):
    flags = kr.FLAGS + (["-fno-slp-vectorize"] if source in kr.NO_SLP else [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "device.s")
        cmd = [kr.find_hipcc(), *flags, f"--offload-arch={arch}", "--cuda-device-only", "-S", source, "-o", out]
        run = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if run.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed in {csrc}:\n{run.stderr[-4000:]}")
        with open(out) as f:
            return f.read()


def kernel_streams(text):
    """{mangled name: normalised lines} -- a kernel's text runs from the directives that open its function (.section, .globl,
    .p2align, .type) over its code and its .amdhsa_kernel descriptor to the symbols the compiler sets behind that."""
    src = text.splitlines()
    end = next((i for i, l in enumerate(src) if ".AMDGPU.gpr_maximums" in l), len(src))
    starts = []
    for i, l in enumerate(src[:end]):
        if _FUNCTION.match(l):
            while i and _OPENING.match(src[i - 1]):
                i -= 1
            starts.append(i)
    streams = {}
    for a, b in zip(starts, starts[1:] + [end]):
        chunk = src[a:b]
        name = next(m.group(1) for m in map(_FUNCTION.match, chunk) if m)      # (a function that is no kernel is compared too)
        labels, lines = {}, []
        for line in chunk:
            line = line.split(";", 1)[0].rstrip()
            if not line.strip() or _DEBUG.match(line):
                continue
            line = line.replace(name, "@kernel").replace("12_GLOBAL__N_1", "")
            line = _LABEL.sub(lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line)
            lines.append(" ".join(line.split()))
        streams[name.replace("12_GLOBAL__N_1", "")] = lines
    return streams


def figures(csrc, source, arch):
    return {k["mangled"].replace("12_GLOBAL__N_1", ""): k for k in kr.kernel_resources(source, arch, csrc=csrc)}


def makefile_sources(csrc):
    with open(os.path.join(csrc, "Makefile")) as f:
        return next(l.split(":=", 1)[1].split() for l in f if re.match(r"SRC\s*:=", l))


def renamed(kernels, maps):
    """The parent's {mangled name: ...} under the --map expressions."""
    out = {}
    for name, value in kernels.items():
        for pattern, repl in maps:
            name = pattern.sub(repl, name)
        if name in out:
            raise SystemExit(f"--map gives two parent kernels the name {name}")
        out[name] = value
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", help="root of the checkout to compare against")
    ap.add_argument("sources", nargs="*", help=f"files of mrla_amd/csrc (default: {' '.join(CONV1X1)})")
    ap.add_argument("--all", action="store_true", help="every source of this checkout's Makefile (its SRC list)")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL",
                    help="re.sub applied to the parent's mangled names before kernels are paired (repeatable)")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), help="this checkout")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    trees = [csrc_of(a.parent), csrc_of(a.tree)]
    sources = a.sources or (makefile_sources(trees[1]) if a.all else CONV1X1)
    maps = [(re.compile(m.split("=", 1)[0]), m.split("=", 1)[1]) for m in a.map]
    jobs = [(t, s) for s in sources for t in trees]
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        asm = dict(zip(jobs, pool.map(lambda j: kernel_streams(assembly(*j, a.arch)), jobs)))
        res = dict(zip(jobs, pool.map(lambda j: figures(*j, a.arch), jobs)))

    bad = total = 0
    print(f"{'file':22s} {'stream':9s} " + " ".join(f"{f:>11s}" for f in FIGURES) + "  kernel   (figures: parent/this)")
    for s in sources:
        old, new = renamed(asm[(trees[0], s)], maps), asm[(trees[1], s)]
        ro, rn = renamed(res[(trees[0], s)], maps), res[(trees[1], s)]
        names = kr.demangle(sorted(set(old) | set(new)))
        same = 0
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                verdict = "ONLY-" + ("THIS" if name in new else "PARENT")
            else:
                verdict = "same" if old[name] == new[name] else "DIFFERS"
            same += verdict == "same"
            bad += verdict != "same"
            cols = " ".join(f"{ro.get(name, {}).get(f, '-')!s:>5s}/{rn.get(name, {}).get(f, '-')!s:<5s}" for f in FIGURES)
            print(f"{s:22s} {verdict:9s} {cols}  {kr.short(names[name])}")
        total += len(new)
        print(f"# {s}: {len(new)} kernels, {same} identical to the parent's", file=sys.stderr)
    print(f"# {total} kernels: {'all instruction streams identical' if not bad else str(bad) + ' differ'}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
