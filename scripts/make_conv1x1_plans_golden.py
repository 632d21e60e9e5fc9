#!/usr/bin/env python3
"""Records tests/golden/conv1x1_plans.json: what the host side of the 1x1-convolution GEMMs answers -- which shapes each
form takes, every integer of a plan, the row counts, and the code of every refused call -- over a grid of shapes, element
types and bad arguments.  tests/test_conv1x1_plans_cpu.py replays the file against the built library, so a change to the
selection of the kernel form, the planners' shared arithmetic or the argument checks shows up as an answer, not as a
differently launched kernel.  Needs the built library, no GPU.

Record it from the library of the commit whose answers are to be kept (MRLA_HIP_LIB selects the library), never from the
change under test:

    MRLA_HIP_LIB=/path/to/parent/libmrla_hip.so python scripts/make_conv1x1_plans_golden.py

Grid.  M: b*h*w of batches 1, 2, 4 .. 256 at 7, 14, 28 and 56 squared (= 49 * 2^j, j = 0 .. 14), and beside them M that
are no multiple of 32 or sit either side of a planner's threshold at n = 2048: 4736 | 4737 (the K-streaming kernel's
larger pixel tile, 300 workgroups), 4864 | 4865 and 5632 | 5633 (its 256 x 256 tile: 160 tiles, 70 % of a round),
262143 | 262144 and 524287 | 524288 (2^31 bytes of fp32 / 16-bit rows of 2048).  K and N: {32, 64, 96, 128, 192, 256, 384,
512, 1024, 2048}, all hundred pairs (n % 256, k 256 | 512 and the unsupported 32, 96 among them).  Thinned, to keep the file
a few hundred KB: bf16 runs the whole grid; fp16, whose plans are the same code, runs every M with K and N from {64, 96, 256,
512, 2048}; MRLA_F32, which every query with a dtype refuses, runs every M with K = N.  Bad arguments: each of m, k, n (and
the strides of the addend query) at 0, -1 and -64 for each dtype, and dtype codes -1, 3, 7 and 100 at eight shapes.

For every query the grid must hold at least FLOOR accepted shapes, FLOOR answers MRLA_EUNSUPPORTED and FLOOR answers
MRLA_EINVAL; main() checks that of the library it records from, the test of the file.

The file holds the answers only, in the order of cases(): a positive integer, the list of a plan's integers, or a code."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv1x1_plans.json")

BF16, F16, F32 = 1, 2, 0                      # MRLA_BF16, MRLA_F16, MRLA_F32 of include/mrla_hip.h
EINVAL, EUNSUPPORTED = -1, -2
FLOOR = 50
MS = sorted({49 << j for j in range(15)} | {33, 100, 1000, 4736, 4737, 4864, 4865, 4999, 5120, 5632, 5633, 12545, 262143,
                                            262144, 524287, 524288})
KN = (32, 64, 96, 128, 192, 256, 384, 512, 1024, 2048)
KN_F16 = (64, 96, 256, 512, 2048)
BAD_EXTENTS = (0, -1, -64)
BAD_DTYPES = (-1, 3, 7, 100)
BASE = [(3136, 64, 256), (3136, 256, 64), (784, 512, 128), (196, 1024, 2048), (12544, 128, 128), (49, 2048, 512),
        (6272, 64, 64), (5120, 1024, 2048)]
# query -> (entry point, takes a dtype, extra arguments behind the dtype, integers of the plan it writes or 0)
QUERIES = {
    "rows": ("mrla_conv1x1_rows", True, (), 0),
    "plan": ("mrla_conv1x1_plan", True, (0,), 4),
    "plan_add": ("mrla_conv1x1_plan", True, (1,), 4),
    "add_supported": ("mrla_conv1x1_add_supported", True, (), 0),
    "addend_supported": ("mrla_conv1x1_addend_supported", True, (), 0),      # (m, k, n, sh, sw, dtype): see call()
    "fwd_affine_supported": ("mrla_conv1x1_fwd_affine_supported", True, (), 0),
    "wgrad_rows": ("mrla_conv1x1_wgrad_rows", True, (), 0),
    "wgrad_plan": ("mrla_conv1x1_wgrad_plan", True, (), 6),
    "wgrad_bn_supported": ("mrla_conv1x1_wgrad_bn_supported", True, (), 0),
    "wgrad_bn_dx_supported": ("mrla_conv1x1_wgrad_bn_dx_supported", True, (), 0),
    "f32_rows": ("mrla_conv1x1_f32_rows", False, (), 0),
    "f32_plan": ("mrla_conv1x1_f32_plan", False, (), 4),
    "f32_wgrad_rows": ("mrla_conv1x1_f32_wgrad_rows", False, (), 0),
}


def cases(query):
    """The argument tuples of a query: (m, k, n, dtype) -- (m, k, n) for the fp32 entries, (m, k, n, sh, sw, dtype) for the
    addend query."""
    _, has_dtype, _, _ = QUERIES[query]
    grid = [(m, k, n) for m in MS for k in KN for n in KN]
    bad = [tuple(v if i == p else x for i, x in enumerate(BASE[0])) for p in range(3) for v in BAD_EXTENTS]
    if not has_dtype:
        return grid + [tuple(v if i == p else x for i, x in enumerate(s)) for s in BASE for p in range(3) for v in BAD_EXTENTS]
    out = [s + (BF16,) for s in grid]
    out += [(m, k, n, F16) for m in MS for k in KN_F16 for n in KN_F16]
    out += [(m, k, k, F32) for m in MS for k in KN]
    out += [s + (d,) for d in (BF16, F16, F32) for s in bad] + [s + (d,) for d in BAD_DTYPES for s in BASE]
    if query == "addend_supported":
        out = [s[:3] + ((1, 1) if i % 3 else (2, 2)) + s[3:] for i, s in enumerate(out)]
        out += [BASE[0] + st + (d,) for d in (BF16, F16, F32) for st in ((0, 1), (1, 0), (-1, 2), (2, -64))]
    return out


def call(lib, query, args):
    """A positive integer, the plan's integers, or the code the entry refuses the arguments with."""
    entry, _, extra, count = QUERIES[query]
    if not count:
        return getattr(lib, entry)(*args, *extra)
    out = (ctypes.c_int * count)()
    rc = getattr(lib, entry)(*args, *extra, ctypes.cast(out, ctypes.c_void_p))
    return list(out) if rc == 0 else rc


def kinds(answers):
    """(accepted, MRLA_EUNSUPPORTED, MRLA_EINVAL) counts; anything else in the answers is an error."""
    ok = sum(isinstance(a, list) or a > 0 for a in answers)
    refused, invalid = answers.count(EUNSUPPORTED), answers.count(EINVAL)
    assert ok + refused + invalid == len(answers), "an answer that is neither accepted nor one of the two codes"
    return ok, refused, invalid


def main():
    from mrla_amd import _lib as L
    assert (L.BF16, L.F16, L.F32, L.EINVAL, L.EUNSUPPORTED) == (BF16, F16, F32, EINVAL, EUNSUPPORTED)
    lib = L.load()
    answers = {q: [call(lib, q, c) for c in cases(q)] for q in QUERIES}
    for q, a in answers.items():
        assert min(kinds(a)) >= FLOOR, (q, kinds(a))
    with open(OUT, "w") as f:
        f.write('{"queries": {\n')
        for i, (q, a) in enumerate(answers.items()):
            lines = [json.dumps(a[k:k + 100], separators=(",", ":"))[1:-1] for k in range(0, len(a), 100)]
            f.write(' "%s": [\n  %s\n ]%s\n' % (q, ",\n  ".join(lines), "," if i + 1 < len(answers) else ""))
        f.write("}}\n")
    print(OUT, os.path.getsize(OUT), "bytes,", {q: kinds(a) for q, a in answers.items()}, "library", L.LIB_PATH)


if __name__ == "__main__":
    main()
