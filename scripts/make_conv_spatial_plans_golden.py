#!/usr/bin/env python3
"""Records tests/golden/conv_spatial_plans.json: what the planners of the three spatial-convolution kernels answer -- the
full output of mrla_conv3x3_wgrad_plan, mrla_conv3x3_fwd_plan and mrla_stem_conv_wgrad_plan and the value of their *_rows
queries, refused shapes with their codes -- over a grid of shapes.  tests/test_conv_spatial_plans_cpu.py replays the file
against the built library, so a change to the planners' shared code that moves any plan shows up as a plan, not as a
slower or differently rounded kernel.  Needs the built library, no GPU.

Record it from the library of the commit whose plans are to be kept (MRLA_HIP_LIB selects the library), never from the
change under test:

    MRLA_HIP_LIB=/path/to/parent/libmrla_hip.so python scripts/make_conv_spatial_plans_golden.py

Grid.  3x3 (both entry points, both strides): b in {1, 2, 8, 256}; (c, n) the four ResNet widths and two c != n pairs;
square maps 1 .. 8 and, of 9 .. 57, the sizes next to where a plan changes form (13 - 15, 27 - 29, 33, 47, 48, 56 - 59: the
ResNet maps, the raster pitch cap of 60 at stride 1), then 70, 112, 117, 119 (the cap at stride 2), 131, 224, 257 and 4000.
Stem: the same b, n in {64, 128}, heights and widths 1 .. 8, 15, 16, 63, 64, 223 - 225, 255 - 257 (the 128-pixel segment),
513 and 2047 -- the squares, and every size against 7 and 224 both ways.  Every map of 1 .. 57 (1 .. 64 for the stem) and
the full cross of heights and widths would make the file several hundred KB, most of a change's diff; the planners are
integer arithmetic in the map size, sampled here on both sides of each threshold.

The file holds the answers only, in the order of shapes(): per shape [rows, plan integers ...], or the code of a refused
shape (which both queries answer)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_spatial_plans.json")

BATCHES = (1, 2, 8, 256)
CHANNELS = ((64, 64), (128, 128), (256, 256), (512, 512), (64, 128), (128, 64))
MAPS = [(m, m) for m in list(range(1, 9)) + [13, 14, 15, 27, 28, 29, 33, 47, 48, 56, 57, 58, 59, 70, 112, 117, 119, 131, 224, 257, 4000]]
STEM_SIZES = list(range(1, 9)) + [15, 16, 63, 64, 223, 224, 225, 255, 256, 257, 513, 2047]
STEM_CROSS = (7, 224)
# entry point -> (rows query, integers of a plan)
ENTRIES = {"mrla_conv3x3_wgrad_plan": ("mrla_conv3x3_wgrad_rows", 6), "mrla_conv3x3_fwd_plan": ("mrla_conv3x3_fwd_rows", 6),
           "mrla_stem_conv_wgrad_plan": ("mrla_stem_conv_wgrad_rows", 7)}


def shapes(entry):
    if entry == "mrla_stem_conv_wgrad_plan":
        maps = [(s, s) for s in STEM_SIZES]
        maps += [(h, w) for h in STEM_SIZES for w in STEM_CROSS if h != w] + [(h, w) for h in STEM_CROSS for w in STEM_SIZES if h != w]
        return [(b, n, h, w) for b in BATCHES for n in (64, 128) for h, w in sorted(set(maps))]
    return [(b, c, n, h, w, s) for b in BATCHES for c, n in CHANNELS for h, w in MAPS for s in (1, 2)]


def answer(lib, entry, shape, dtype):
    """[rows, plan integers ...] of `entry` for `shape`, or the one code both queries refuse it with."""
    rows_entry, count = ENTRIES[entry]
    out = (ctypes.c_int * count)()
    rc = getattr(lib, entry)(*shape, dtype, ctypes.cast(out, ctypes.c_void_p))
    rows = getattr(lib, rows_entry)(*shape, dtype)
    assert (rc == 0) == (rows > 0) and (rc == 0 or rows == rc), (entry, shape, rows, rc)
    return [rows] + list(out) if rc == 0 else rc


def main():
    from mrla_amd import _lib as L
    lib = L.load()
    answers = {e: [answer(lib, e, s, L.BF16) for s in shapes(e)] for e in ENTRIES}
    per_line = 2 * len(MAPS)
    with open(OUT, "w") as f:
        f.write('{"dtype": %d, "entries": {\n' % L.BF16)
        for i, (e, a) in enumerate(answers.items()):
            lines = [json.dumps(a[k:k + per_line], separators=(",", ":"))[1:-1] for k in range(0, len(a), per_line)]
            f.write(' "%s": [\n  %s\n ]%s\n' % (e, ",\n  ".join(lines), "," if i + 1 < len(answers) else ""))
        f.write("}}\n")
    print(OUT, os.path.getsize(OUT), "bytes,", {e: len(a) for e, a in answers.items()}, "cases, library", L.LIB_PATH)


if __name__ == "__main__":
    main()
