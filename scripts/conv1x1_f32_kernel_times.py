"""Per-kernel device time of the fp32 1x1-convolution GEMMs (mrla_conv1x1_f32_fwd / _wgrad) against what the stock route
launches for the same thing (MIOpen's convolution + mrla_bn_plane_moments, aten.convolution_backward), for conv1 / conv3 /
downsample of each ResNet-50 stage at batch 64 and 256: the table of profiles/conv1x1_f32.md section 3.
    python scripts/conv1x1_f32_kernel_times.py [out.jsonl]
HIP events around N_LAUNCH back-to-back launches, ROUNDS rounds, the two sides alternating; median, min and max of the
per-launch time in microseconds; bytes = 4 (mk + mn + nk), flop = 2 mkn."""
import json, statistics, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mrla_amd import _lib as L

torch.backends.cudnn.benchmark = True
lib = L.load()
CL = torch.channels_last
N_LAUNCH, ROUNDS = 10, 5
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N_LAUNCH):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / N_LAUNCH        # us per launch


def ab(fa, fb):
    fa(); fb(); fa(); fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(timed(fa)); b.append(timed(fb))
    return a, b


def stat(v):
    return dict(med=round(statistics.median(v), 1), lo=round(min(v), 1), hi=round(max(v), 1))


def shapes(batch):
    res, inpl, hw = [], 64, 56
    for stage, p in enumerate((64, 128, 256, 512)):
        if stage:
            hw //= 2
        m = batch * hw * hw
        res += [(f"s{stage+1}.conv1", batch, hw, 4 * p, p), (f"s{stage+1}.conv3", batch, hw, p, 4 * p),
                (f"s{stage+1}.down", batch, hw, inpl, 4 * p)]
        inpl = 4 * p
    return res


st = torch.cuda.current_stream().cuda_stream
for batch in (64, 256):
    for name, b, hw, k, n in shapes(batch):
        m = b * hw * hw
        x = torch.randn(b, k, hw, hw, device="cuda").contiguous(memory_format=CL)
        w = (torch.randn(n, k, 1, 1, device="cuda") * (2.0 / k) ** 0.5).contiguous(memory_format=CL)
        dy = torch.randn(b, n, hw, hw, device="cuda").contiguous(memory_format=CL)
        y = torch.empty(b, n, hw, hw, device="cuda").contiguous(memory_format=CL)
        dx = torch.empty_like(x)
        dw = torch.empty(n, k, device="cuda")
        rows = lib.mrla_conv1x1_f32_rows(m, k, n)
        part = torch.empty(rows, n, 4, device="cuda")
        wrows = lib.mrla_conv1x1_f32_wgrad_rows(m, k, n)
        wpart = torch.empty(wrows, n, k, device="cuda")
        brows = lib.mrla_bn_moment_rows(b, n, hw, hw, L.NHWC)
        amom = torch.empty(brows, n, 2, device="cuda")
        pivot = torch.empty(n, device="cuda")

        def new_fwd():
            L.call("mrla_conv1x1_f32_fwd", x.data_ptr(), w.data_ptr(), 0, y.data_ptr(), part.data_ptr(), m, k, n, st)

        def old_fwd():
            yy = torch.nn.functional.conv2d(x, w)
            L.call("mrla_bn_plane_moments", yy.data_ptr(), amom.data_ptr(), pivot.data_ptr(), b, n, hw, hw, L.F32, L.NHWC, st)

        def old_fwd_conv_only():
            torch.nn.functional.conv2d(x, w)

        def new_dx():
            L.call("mrla_conv1x1_f32_fwd", dy.data_ptr(), w.data_ptr(), 1, dx.data_ptr(), None, m, n, k, st)

        def old_dx():
            torch.ops.aten.convolution_backward(dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, [True, False, False])

        def new_dw():
            L.call("mrla_conv1x1_f32_wgrad", dy.data_ptr(), x.data_ptr(), wpart.data_ptr(), dw.data_ptr(), m, k, n, st)

        def old_dw():
            torch.ops.aten.convolution_backward(dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, [False, True, False])

        flop = 2.0 * m * k * n
        for op, fa, fb, byts in (("fwd+records", new_fwd, old_fwd, 4.0 * (m * k + m * n + n * k)),
                                 ("fwd_conv_only", new_fwd, old_fwd_conv_only, 4.0 * (m * k + m * n + n * k)),
                                 ("dX", new_dx, old_dx, 4.0 * (m * k + m * n + n * k)),
                                 ("dW", new_dw, old_dw, 4.0 * (m * k + m * n + n * k))):
            a, o = ab(fa, fb)
            sa, so = stat(a), stat(o)
            rec = dict(shape=name, batch=b, m=m, k=k, n=n, op=op, new_us=sa, old_us=so, new_TBps=round(byts / sa["med"] / 1e6, 2),
                       new_TF=round(flop / sa["med"] / 1e6, 1), speedup=round(so["med"] / sa["med"], 2))
            out.write(json.dumps(rec) + "\n"); out.flush()
            print(f"b{b:<3d} {name:9s} m={m:<7d} k={k:<4d} n={n:<4d} {op:13s} new {sa['med']:8.1f} us [{sa['lo']:.1f}-{sa['hi']:.1f}]  "
                  f"old {so['med']:8.1f} us [{so['lo']:.1f}-{so['hi']:.1f}]  x{rec['speedup']:.2f}  {rec['new_TBps']:.2f} TB/s {rec['new_TF']:.1f} TF", flush=True)
        del x, w, dy, y, dx, part, wpart
        torch.cuda.empty_cache()
