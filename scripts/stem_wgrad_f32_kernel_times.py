"""Per-shape device time of the fp32 stem weight gradient: mrla_stem_conv_f32_wgrad (its kernel + its reduction) against
EVERYTHING the stock operator launches for the same gradient in fp32 (zero-fill, solver, layout kernels), from kernel traces --
the table of profiles/stem_wgrad_f32.md.  One profiler run per side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/stem_wgrad_f32_kernel_times.py run own
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/stem_wgrad_f32_kernel_times.py run stock
    python scripts/stem_wgrad_f32_kernel_times.py table OUT/own OUT/stock

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a marker.
`table` cuts each trace at the markers and prints, per shape, the device time per launch of the N timed launches, the own
side's TF -- of the 2 * 147 * b * ho * wo * n useful flop, and of the 2 * 192 * b * ho * wo * n the padded product issues --
over kernel + reduction, the latter's share of the 157.3 TF fp32 MFMA peak, and the kernels the stock side consisted of.
Shapes: 3 -> 64 channels at batch 256 / 64 / 16 of 224 x 224 images and 2 images of 800 x 1344.  fp32 everywhere; the stock side
is aten.convolution_backward with output_mask (False, True, False) on the fp32 weight, in find mode, as the fp32 recipe reaches
it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv3x3_wgrad_kernel_times as base  # noqa: E402  (the trace reader is shared)

WARM, N = base.WARM, base.N
PEAK_TF = 157.3       # the specified fp32 MFMA peak (256 CUs x 4 SIMDs x 64 flop / clock x 2.4 GHz), as in profiles/conv3x3_wgrad_f32.md;
#                       155 TF is what the instruction has been measured to reach
SHAPES = [(f"b{b} 3->64 {h}x{w}", b, 64, h, w) for b, h, w in ((256, 224, 224), (64, 224, 224), (16, 224, 224), (2, 800, 1344))]


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock side as the training recipe runs it (find mode)
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    mark = torch.full((64,), 0.5, device="cuda")
    for name, b, n, h, wd in SHAPES:
        ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
        x = torch.randn(b, 3, h, wd, device="cuda").contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, wo, device="cuda").contiguous(memory_format=CL)
        w = torch.randn(n, 3, 7, 7, device="cuda").contiguous(memory_format=CL)
        rows = L.load().mrla_stem_conv_f32_wgrad_rows(b, n, h, wd)
        part = torch.empty(rows, n, 147, device="cuda")
        dw = torch.empty(n, 3, 7, 7, device="cuda").contiguous(memory_format=CL)

        def own():
            L.call("mrla_stem_conv_f32_wgrad", dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), b, n, h, wd, st)

        def stock():
            return torch.ops.aten.convolution_backward(dy, x, w, None, (2, 2), (3, 3), (1, 1), False, (0, 0), 1,
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
    print("| shape | own us | kernel | reduction | useful TF | issued TF | of peak | stock us | own / stock | stock kernels per launch |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (name, b, n, h, wd), o, t in zip(SHAPES, own, stock):
        assert len(o) == 2 * N, (name, len(o))
        main = sum(ns for k, ns in o if "split_sum" not in k) / N / 1e3
        red = sum(ns for k, ns in o if "split_sum" in k) / N / 1e3
        m = b * ((h - 1) // 2 + 1) * ((wd - 1) // 2 + 1)
        tf = [2.0 * cols * m * n / ((main + red) * 1e-6) / 1e12 for cols in (147, 192)]
        st = sum(ns for _, ns in t) / N / 1e3
        kinds = {}
        for k, ns in t:
            e = kinds.setdefault(base.short(k), [0, 0])
            e[0] += 1
            e[1] += ns
        desc = "; ".join(f"{cnt / N:g} x {k} ({ns / N / 1e3:.1f})" for k, (cnt, ns) in sorted(kinds.items(), key=lambda kv: -kv[1][1]))
        print(f"| {name} | {main + red:.1f} | {main:.1f} | {red:.1f} | {tf[0]:.1f} | {tf[1]:.1f} | {100 * tf[1] / PEAK_TF:.0f} % | "
              f"{st:.1f} | {(main + red) / st:.2f} | {desc} |")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(sys.argv[2], sys.argv[3])
