"""Per-shape device time of the 3x3 weight gradient: mrla_conv3x3_wgrad (its kernel + its reduction) against EVERYTHING the
stock operator launches for the same gradient (zero-fill, solver, cast, layout kernels), from kernel traces -- the table of
profiles/conv3x3_wgrad.md.  One profiler run per side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/conv3x3_wgrad_kernel_times.py run own
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/conv3x3_wgrad_kernel_times.py run stock
    python scripts/conv3x3_wgrad_kernel_times.py table OUT/own OUT/stock

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a marker.
`table` cuts each trace at the markers and prints, per shape, the device time per launch of the N timed launches and the
kernels they consisted of.  Shapes: the seven 3x3 convolutions of ResNet-50 at batch 256, 128, 64 and 32 (what the rule of
mrla_conv3x3_wgrad_preferred rests on) and the two shapes at which the stock gradient is wrong under graph replay, at batch 8
and 16.  bf16, fp32 dw on the own side (what the route asks for); the stock side is aten.convolution_backward with output_mask
(False, True, False) on the bf16 weight, as autocast reaches it.

The own side binds the two entry points it calls itself, from MRLA_HIP_LIB where that is set: another build of the library --
an older one, which lacks symbols the package binds, included -- is timed by the same command, one process per library:

    MRLA_HIP_LIB=/path/to/other/libmrla_hip.so rocprofv3 ... -d OUT/other -- python scripts/conv3x3_wgrad_kernel_times.py run own
    python scripts/conv3x3_wgrad_kernel_times.py table OUT/own OUT/stock OUT/other      # one more column: the other build"""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, N = 3, 10
RESNET50 = ((64, 56, 1), (128, 56, 2), (128, 28, 1), (256, 28, 2), (256, 14, 1), (512, 14, 2), (512, 7, 1))
SHAPES = [(f"b{b} {c}->{n} {h}x{h} s{s}", b, c, n, h, s) for b, c, n, h, s in (
    *((b, c, c, h, s) for b in (256, 128, 64, 32) for c, h, s in RESNET50), (8, 512, 512, 7, 1), (16, 512, 512, 7, 1),
    (8, 512, 512, 14, 2), (16, 512, 512, 14, 2))]


def own_entry_points():
    """(rows, launch) of the library at MRLA_HIP_LIB, else the package's own -- bound here, not through mrla_amd._lib, which
    insists on every symbol of ITS header."""
    import ctypes

    import torch  # noqa: F401  (first: the library's HIP runtime must be the one torch brought into the process)
    from mrla_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("mrla_conv3x3_wgrad_rows", "mrla_conv3x3_wgrad"):
        getattr(lib, name).argtypes = L.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib.mrla_conv3x3_wgrad_rows, lib.mrla_conv3x3_wgrad


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock side as the training recipe runs it (find mode)
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    mark = torch.full((64,), 0.5, device="cuda")
    wgrad_rows, wgrad = own_entry_points()
    for name, b, c, n, h, s in SHAPES:
        ho = (h - 1) // s + 1
        x = torch.randn(b, c, h, h, device="cuda").bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, ho, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = torch.randn(n, c, 3, 3, device="cuda").bfloat16().contiguous(memory_format=CL)
        rows = wgrad_rows(b, c, n, h, h, s, L.BF16)
        part = torch.empty(rows, n, 9, c, device="cuda")
        dw = torch.empty(n, c, 3, 3, device="cuda").contiguous(memory_format=CL)

        def own():
            L.check(wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), b, c, n, h, h, s, L.BF16, L.F32, st),
                    "mrla_conv3x3_wgrad")

        def stock():
            g = torch.ops.aten.convolution_backward(dy, x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), 1,
                                                    [False, True, False])[1]
            return g.float()                            # (the cast autograd appends for an fp32 master weight)
        fn = own if side == "own" else stock
        torch.cuda.synchronize()
        torch.erfinv(mark)
        for _ in range(WARM):
            fn()
        torch.erfinv(mark)
        for _ in range(N):
            fn()
        torch.erfinv(mark)
        torch.cuda.synchronize()
        del x, dy, w, part, dw
        torch.cuda.empty_cache()


def segments(directory):
    """[[(kernel name, ns), ...] per timed window] of the kernel trace under `directory`, in launch order."""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    recs = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                r = {k.lower(): v for k, v in r.items()}
                recs.append((int(r["start_timestamp"]), int(r["end_timestamp"]) - int(r["start_timestamp"]), r["kernel_name"]))
    recs.sort()
    cuts, cur = [], None
    for _, ns, name in recs:
        if "erfinv" in name:
            if cur is not None:
                cuts.append(cur)
            cur = []
        elif cur is not None:
            cur.append((name, ns))
    assert len(cuts) == 3 * len(SHAPES) - 1, (len(cuts), len(SHAPES))
    return [cuts[3 * i + 1] for i in range(len(SHAPES))]          # (warm-up, TIMED, gap to the next shape) per shape


def short(name):
    name = name.split("(")[0]
    return name if len(name) <= 60 else name[:57] + "..."


def table(own_dir, stock_dir, other_dir=None):
    own, stock = segments(own_dir), segments(stock_dir)
    other = segments(other_dir) if other_dir else [None] * len(SHAPES)
    print("| shape | own us | kernel | reduction | stock us | own / stock | stock kernels per launch |"
          + (" other build: kernel | kernel / other |" if other_dir else ""))
    print("|---|---|---|---|---|---|---|" + ("---|---|" if other_dir else ""))
    for (name, *_), o, s, t in zip(SHAPES, own, stock, other):
        assert len(o) == 2 * N, (name, len(o))
        main = sum(ns for k, ns in o if "split_sum" not in k) / N / 1e3
        red = sum(ns for k, ns in o if "split_sum" in k) / N / 1e3
        tail = ""
        if t is not None:
            assert len(t) == 2 * N, (name, len(t))
            tmain = sum(ns for k, ns in t if "split_sum" not in k) / N / 1e3
            tail = f" {tmain:.1f} | {main / tmain:.2f} |"
        st = sum(ns for _, ns in s) / N / 1e3
        kinds = {}
        for k, ns in s:
            e = kinds.setdefault(short(k), [0, 0])
            e[0] += 1
            e[1] += ns
        desc = "; ".join(f"{cnt / N:g} x {k} ({ns / N / 1e3:.1f})" for k, (cnt, ns) in sorted(kinds.items(), key=lambda kv: -kv[1][1]))
        print(f"| {name} | {main + red:.1f} | {main:.1f} | {red:.1f} | {st:.1f} | {(main + red) / st:.2f} | {desc} |" + tail)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(*sys.argv[2:5])
