"""Per-shape device time of the own stride-2 3x3 input gradient (mrla_conv3x3_dgrad_s2) against EVERYTHING the stock operator
launches for the same result, from kernel traces -- the tables of profiles/conv3x3_dgrad.md.  One profiler run per side, no
counters in it, each under a time limit of its own:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/conv3x3_dgrad_kernel_times.py run own
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/conv3x3_dgrad_kernel_times.py run stock
    python scripts/conv3x3_dgrad_kernel_times.py table OUT/own OUT/stock

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a
marker.  `table` cuts each trace at the markers and prints the device time per launch of the N timed launches and the kernels
they consisted of.  own: mrla_conv3x3_dgrad_s2 on dy and the forward's own weight (no permutation in front of it); stock:
aten.convolution_backward with output_mask (True, False, False), in find mode as the training recipe runs it.  Shapes: the
three stride-2 3x3 convolutions of ResNet-50 at batch 256, and the last of them at batch 8.  bf16."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, N = 3, 10
SHAPES = [(f"b{b} {c}->{n} {h}x{h} s2", b, c, n, h) for b, c, n, h in (
    (256, 128, 128, 56), (256, 256, 256, 28), (256, 512, 512, 14), (8, 512, 512, 14))]
WINDOWS = [(name, "dx") for name, *_ in SHAPES]


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock side as the training recipe runs it (find mode)
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    mark = torch.full((64,), 0.5, device="cuda")
    for name, b, c, n, h in SHAPES:
        ho = (h - 1) // 2 + 1
        x = torch.randn(b, c, h, h, device="cuda").bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, ho, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(n, c, 3, 3, device="cuda") * (2.0 / (9 * c)) ** 0.5).bfloat16().contiguous(memory_format=CL)
        dx = torch.empty_like(x)

        def own_dx():
            L.call("mrla_conv3x3_dgrad_s2", dy.data_ptr(), w.data_ptr(), dx.data_ptr(), b, c, n, h, h, L.BF16, st)

        def stock_dx():
            return torch.ops.aten.convolution_backward(dy, x, w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1,
                                                       [True, False, False])[0]
        fn = own_dx if side == "own" else stock_dx
        torch.cuda.synchronize()
        torch.erfinv(mark)
        for _ in range(WARM):
            fn()
        torch.erfinv(mark)
        for _ in range(N):
            fn()
        torch.erfinv(mark)
        torch.cuda.synchronize()
        del x, dy, w, dx
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
