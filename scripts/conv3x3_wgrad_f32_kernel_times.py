"""Per-shape device time of the fp32 3x3 weight gradient: mrla_conv3x3_f32_wgrad (its kernel + its reduction) against EVERYTHING
the stock operator launches for the same gradient in fp32 (zero-fill, solver, layout kernels), from kernel traces -- the table
of profiles/conv3x3_wgrad_f32.md.  One profiler run per side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/conv3x3_wgrad_f32_kernel_times.py run own
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/conv3x3_wgrad_f32_kernel_times.py run stock
    python scripts/conv3x3_wgrad_f32_kernel_times.py table OUT/own OUT/stock

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a marker.
`table` cuts each trace at the markers and prints, per shape, the device time per launch of the N timed launches, the own
side's TF (2 * 9 * b * ho * wo * n * c flop over kernel + reduction) and its share of the 157.3 TF fp32 MFMA peak, and the
kernels the stock side consisted of.  Shapes: the seven 3x3 convolutions of ResNet-50 at batch 64 and 256, and the two batch-8
shapes of the replay tests.  fp32 everywhere; the stock side is aten.convolution_backward with output_mask (False, True, False)
on the fp32 weight, in find mode, as the fp32 recipe reaches it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv3x3_wgrad_kernel_times as base  # noqa: E402  (the trace reader is shared)

WARM, N = base.WARM, base.N
PEAK_TF = 157.3
SHAPES = [(f"b{b} {c}->{n} {h}x{h} s{s}", b, c, n, h, s) for b, c, n, h, s in (
    *((b, c, c, h, s) for b in (64, 256) for c, h, s in base.RESNET50), (8, 512, 512, 7, 1), (8, 512, 512, 14, 2))]


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock side as the training recipe runs it (find mode)
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    mark = torch.full((64,), 0.5, device="cuda")
    for name, b, c, n, h, s in SHAPES:
        ho = (h - 1) // s + 1
        x = torch.randn(b, c, h, h, device="cuda").contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, ho, device="cuda").contiguous(memory_format=CL)
        w = torch.randn(n, c, 3, 3, device="cuda").contiguous(memory_format=CL)
        rows = L.load().mrla_conv3x3_f32_wgrad_rows(b, c, n, h, h, s)
        part = torch.empty(rows, n, 9, c, device="cuda")
        dw = torch.empty(n, c, 3, 3, device="cuda").contiguous(memory_format=CL)

        def own():
            L.call("mrla_conv3x3_f32_wgrad", dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), b, c, n, h, h, s, st)

        def stock():
            return torch.ops.aten.convolution_backward(dy, x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), 1,
                                                       [False, True, False])[1]
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


def table(own_dir, stock_dir):
    base.SHAPES = SHAPES                                 # (segments() counts the windows by it)
    own, stock = base.segments(own_dir), base.segments(stock_dir)
    print("| shape | own us | kernel | reduction | own TF | of peak | stock us | own / stock | stock kernels per launch |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (name, b, c, n, h, s), o, t in zip(SHAPES, own, stock):
        assert len(o) == 2 * N, (name, len(o))
        main = sum(ns for k, ns in o if "split_sum" not in k) / N / 1e3
        red = sum(ns for k, ns in o if "split_sum" in k) / N / 1e3
        ho = (h - 1) // s + 1
        tf = 2.0 * 9 * b * ho * ho * n * c / ((main + red) * 1e-6) / 1e12
        st = sum(ns for _, ns in t) / N / 1e3
        kinds = {}
        for k, ns in t:
            e = kinds.setdefault(base.short(k), [0, 0])
            e[0] += 1
            e[1] += ns
        desc = "; ".join(f"{cnt / N:g} x {k} ({ns / N / 1e3:.1f})" for k, (cnt, ns) in sorted(kinds.items(), key=lambda kv: -kv[1][1]))
        print(f"| {name} | {main + red:.1f} | {main:.1f} | {red:.1f} | {tf:.1f} | {100 * tf / PEAK_TF:.0f} % | {st:.1f} | "
              f"{(main + red) / st:.2f} | {desc} |")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(sys.argv[2], sys.argv[3])
