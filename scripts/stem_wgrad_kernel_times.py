"""Per-shape device time of the stem's weight gradient: mrla_stem_conv_wgrad (its kernel + its reduction) against EVERYTHING
the stock operator launches for the same gradient (zero-fill, solver, cast, layout kernels), from kernel traces -- the table
of profiles/stem_wgrad.md.  One profiler run per side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/own   -- python scripts/stem_wgrad_kernel_times.py run own
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/stem_wgrad_kernel_times.py run stock
    python scripts/stem_wgrad_kernel_times.py table OUT/own OUT/stock

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a marker.
`table` cuts each trace at the markers and prints, per shape, the device time per launch of the N timed launches and the
kernels they consisted of.  Shapes: 3 -> 64 channels at batch 256 / 64 / 16 of 224 x 224 images and 2 images of 800 x 1344.
bf16, fp32 dw on the own side (what the route asks for); the stock side is aten.convolution_backward with output_mask
(False, True, False) on the bf16 weight, as autocast reaches it, plus the cast to fp32."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conv3x3_wgrad_kernel_times as base  # noqa: E402  (the trace reader and the table are shared)

WARM, N = base.WARM, base.N
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
        x = torch.randn(b, 3, h, wd, device="cuda").bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(b, n, ho, wo, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = torch.randn(n, 3, 7, 7, device="cuda").bfloat16().contiguous(memory_format=CL)
        rows = L.load().mrla_stem_conv_wgrad_rows(b, n, h, wd, L.BF16)
        part = torch.empty(rows, n, 147, device="cuda")
        dw = torch.empty(n, 3, 7, 7, device="cuda").contiguous(memory_format=CL)

        def own():
            L.call("mrla_stem_conv_wgrad", dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), b, n, h, wd, L.BF16, L.F32, st)

        def stock():
            g = torch.ops.aten.convolution_backward(dy, x, w, None, (2, 2), (3, 3), (1, 1), False, (0, 0), 1,
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


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        base.SHAPES = SHAPES                             # (segments() and table() count and name the windows by it)
        base.table(sys.argv[2], sys.argv[3])
