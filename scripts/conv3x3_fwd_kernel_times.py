"""Per-shape device time of the own 3x3 forward and stride-1 input gradient (mrla_conv3x3_fwd) against EVERYTHING the stock
operator launches for the same result, from kernel traces -- the tables of profiles/conv3x3_fwd.md.  One profiler run per
side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/conv3x3_fwd_kernel_times.py run own
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/conv3x3_fwd_kernel_times.py run stock
    python scripts/conv3x3_fwd_kernel_times.py table OUT/own OUT/stock

`run` launches, per (shape, product): a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N
launches, a marker.  `table` cuts each trace at the markers and prints the device time per launch of the N timed launches and
the kernels they consisted of.  Products: `fwd` = the convolution with the BatchNorm moments of its output (own: one kernel that
writes the records; stock: aten.convolution, then the moments pass mrla_bn_plane_moments that reads y back), `dx` = the input
gradient at stride 1 (own: the same kernel on the flipped, transposed weight, the permutation included; stock:
aten.convolution_backward with output_mask (True, False, False)).  Shapes: the seven 3x3 convolutions of ResNet-50 at batch 256,
and batch 8 and 16 at 512 channels.  bf16."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, N = 3, 10
SHAPES = [(f"b{b} {c}->{n} {h}x{h} s{s}", b, c, n, h, s) for b, c, n, h, s in (
    (256, 64, 64, 56, 1), (256, 128, 128, 56, 2), (256, 128, 128, 28, 1), (256, 256, 256, 28, 2), (256, 256, 256, 14, 1),
    (256, 512, 512, 14, 2), (256, 512, 512, 7, 1), (8, 512, 512, 7, 1), (16, 512, 512, 7, 1))]
WINDOWS = [(name, kind) for name, *_, s in SHAPES for kind in (("fwd", "dx") if s == 1 else ("fwd",))]


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock side as the training recipe runs it (find mode)
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    mark = torch.full((64,), 0.5, device="cuda")
    for name, b, c, n, h, s in SHAPES:
        ho = (h - 1) // s + 1
        x = torch.randn(b, c, h, h, device="cuda").bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, ho, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(n, c, 3, 3, device="cuda") * (2.0 / (9 * c)) ** 0.5).bfloat16().contiguous(memory_format=CL)
        y = torch.empty(b, n, ho, ho, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
        dx = torch.empty_like(x)
        rows = L.load().mrla_conv3x3_fwd_rows(b, c, n, h, h, s, L.BF16)
        rec = torch.empty(rows, n, L.GEMM_MOMENTS, device="cuda")
        prow = L.load().mrla_bn_moment_rows(b, n, ho, ho, L.NHWC)
        amom, pivot = torch.empty(prow, n, 2, device="cuda"), torch.empty(n, device="cuda")

        def own_fwd():
            L.call("mrla_conv3x3_fwd", x.data_ptr(), w.data_ptr(), y.data_ptr(), rec.data_ptr(), b, c, n, h, h, s, L.BF16, st)

        def stock_fwd():
            out = torch.ops.aten.convolution(x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), 1)
            L.call("mrla_bn_plane_moments", out.data_ptr(), amom.data_ptr(), pivot.data_ptr(), b, n, ho, ho, L.BF16, L.NHWC, st)

        def own_dx():
            wflip = w.flip(2, 3).transpose(0, 1).contiguous(memory_format=CL)
            L.call("mrla_conv3x3_fwd", dy.data_ptr(), wflip.data_ptr(), dx.data_ptr(), None, b, n, c, h, h, 1, L.BF16, st)

        def stock_dx():
            return torch.ops.aten.convolution_backward(dy, x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), 1,
                                                       [True, False, False])[0]
        for kind in (("fwd", "dx") if s == 1 else ("fwd",)):
            fn = {("own", "fwd"): own_fwd, ("stock", "fwd"): stock_fwd, ("own", "dx"): own_dx, ("stock", "dx"): stock_dx}[side, kind]
            torch.cuda.synchronize()
            torch.erfinv(mark)
            for _ in range(WARM):
                fn()
            torch.erfinv(mark)
            for _ in range(N):
                fn()
            torch.erfinv(mark)
            torch.cuda.synchronize()
        del x, dy, w, y, dx, rec, amom, pivot
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
    assert len(cuts) == 3 * len(WINDOWS) - 1, (len(cuts), len(WINDOWS))
    return [cuts[3 * i + 1] for i in range(len(WINDOWS))]         # (warm-up, TIMED, gap to the next window) per window


def short(name):
    name = name.split("(")[0]
    return name if len(name) <= 60 else name[:57] + "..."


def kinds_of(seg):
    kinds = {}
    for k, ns in seg:
        e = kinds.setdefault(short(k), [0, 0])
        e[0] += 1
        e[1] += ns
    return "; ".join(f"{cnt / N:g} x {k} ({ns / N / 1e3:.1f})" for k, (cnt, ns) in sorted(kinds.items(), key=lambda kv: -kv[1][1]))


def table(own_dir, stock_dir):
    own, stock = segments(own_dir), segments(stock_dir)
    print("| shape | product | own us | stock us | own / stock | own kernels per launch | stock kernels per launch |")
    print("|---|---|---|---|---|---|---|")
    for (name, kind), o, s in zip(WINDOWS, own, stock):
        ot, st = sum(ns for _, ns in o) / N / 1e3, sum(ns for _, ns in s) / N / 1e3
        print(f"| {name} | {kind} | {ot:.1f} | {st:.1f} | {ot / st:.2f} | {kinds_of(o)} | {kinds_of(s)} |")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(sys.argv[2], sys.argv[3])
