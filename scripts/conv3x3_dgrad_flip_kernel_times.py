"""Per-shape device time of the stride-1 3x3 input gradient as the stock FORWARD convolution on the banked flipped weight
(CONV3X3_DGRAD_FLIP) against EVERYTHING aten.convolution_backward launches for the same gradient, from kernel traces -- the
table of profiles/conv3x3_dgrad_flip.md section 1, which mrla_conv3x3_dgrad_flip_preferred rests on.  One profiler run per
side, no counters in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/flip  -- python scripts/conv3x3_dgrad_flip_kernel_times.py run flip
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/stock -- python scripts/conv3x3_dgrad_flip_kernel_times.py run stock
    python scripts/conv3x3_dgrad_flip_kernel_times.py table OUT/flip OUT/stock [OUT/flip2 OUT/stock2]

`run` launches, per shape: a marker kernel (erfinv: nothing else here launches it), WARM launches, a marker, N launches, a
marker; the flip side ends with one more window, the refresh of the thirteen routed weights of ResNet-50
(mrla_conv3x3_weight_bank_refresh), whose time the table spreads over those thirteen convolutions.  `table` cuts each trace at
the markers and prints the device time per launch; with a second pair of traces also the run-to-run spread of each side and
whether the flip side wins by more than twice the larger one.  Shapes (c == n, bf16): the four stride-1 3x3 convolutions of
ResNet-50 at batch 32, 64, 96, 128 and 256 (batch 128: also those of resnet101_mrlab's step) and those of the detection
backbone on 2 x 3 x 800 x 1344 images."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, N = 3, 10
WIDTHS = ((64, 56), (128, 28), (256, 14), (512, 7))
SHAPES = [(f"b{b} {c}->{c} {h}x{h}", b, c, h, h) for b in (32, 64, 96, 128, 256) for c, h in WIDTHS]
SHAPES += [(f"b2 {c}->{c} {h}x{w} (detection)", 2, c, h, w) for c, h, w in ((64, 200, 336), (128, 100, 168), (256, 50, 84),
                                                                          (512, 25, 42))]
BANK = [64] * 3 + [128] * 3 + [256] * 5 + [512] * 2              # the routed convolutions of one resnet50_mrlal step
REFRESH = "refresh of 13 weights"


def windows(side):
    return [name for name, *_ in SHAPES] + ([REFRESH] if side == "flip" else [])


def run(side):
    import torch
    from mrla_amd import _lib as L
    torch.backends.cudnn.benchmark = True               # the stock library as the training recipe runs it (find mode)
    CL = torch.channels_last
    mark = torch.full((64,), 0.5, device="cuda")

    def window(fn):
        torch.cuda.synchronize()
        torch.erfinv(mark)
        for _ in range(WARM):
            fn()
        torch.erfinv(mark)
        for _ in range(N):
            fn()
        torch.erfinv(mark)
        torch.cuda.synchronize()

    for name, b, c, h, w in SHAPES:
        x = torch.randn(b, c, h, w, device="cuda").bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(b, c, h, w, device="cuda").bfloat16().contiguous(memory_format=CL)
        w16 = (torch.randn(c, c, 3, 3, device="cuda") * (2.0 / (9 * c)) ** 0.5).bfloat16().contiguous(memory_format=CL)
        wflip = w16.flip(2, 3).transpose(0, 1).contiguous(memory_format=CL)
        if side == "flip":
            window(lambda: torch.ops.aten.convolution(dy, wflip, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1))
        else:
            window(lambda: torch.ops.aten.convolution_backward(dy, x, w16, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                               [True, False, False]))
        del x, dy, w16, wflip
        torch.cuda.empty_cache()
    if side == "flip":
        masters = [torch.randn(c, c, 3, 3, device="cuda").contiguous(memory_format=CL) for c in BANK]
        copies = [(torch.empty_like(m, dtype=torch.bfloat16), torch.empty_like(m, dtype=torch.bfloat16)) for m in masters]
        table = torch.tensor([[m.data_ptr(), a.data_ptr(), f.data_ptr(), (m.shape[0] << 32) | m.shape[1], 1]
                              for m, (a, f) in zip(masters, copies)], dtype=torch.int64).cuda()
        tiles = max(9 * (c // 64) ** 2 for c in BANK)
        st = torch.cuda.current_stream().cuda_stream
        window(lambda: L.call("mrla_conv3x3_weight_bank_refresh", table.data_ptr(), len(BANK), tiles, L.BF16, st))


def segments(directory, side):
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
    n = len(windows(side))
    assert len(cuts) == 3 * n - 1, (len(cuts), n)
    return [cuts[3 * i + 1] for i in range(n)]         # (warm-up, TIMED, gap to the next window) per window


def short(name):
    name = name.split("(")[0]
    return name if len(name) <= 48 else name[:45] + "..."


def kinds_of(seg):
    kinds = {}
    for k, ns in seg:
        e = kinds.setdefault(short(k), [0, 0])
        e[0] += 1
        e[1] += ns
    return "; ".join(f"{cnt / N:g} x {k} ({ns / N / 1e3:.1f})" for k, (cnt, ns) in sorted(kinds.items(), key=lambda kv: -kv[1][1]))


def us(seg):
    return sum(ns for _, ns in seg) / N / 1e3


def table(dirs):
    flips = [segments(d, "flip") for d in dirs[0::2]]
    stocks = [segments(d, "stock") for d in dirs[1::2]]
    share = [us(f[-1]) / len(BANK) for f in flips]
    print(f"refresh of {len(BANK)} weights: " + ", ".join(f"{s * len(BANK):.1f}" for s in share) + " us per launch = "
          + ", ".join(f"{s:.2f}" for s in share) + " us per convolution")
    print("| shape | stock us (runs) | flip us + refresh share (runs) | difference | spread stock / flip | wins by > 2 x spread | "
          "stock kernels per launch | flip kernels per launch |")
    print("|---|---|---|---|---|---|---|---|")
    for i, (name, *_) in enumerate(SHAPES):
        s = [us(r[i]) for r in stocks]
        f = [us(r[i]) + sh for r, sh in zip(flips, share)]
        diff = sum(s) / len(s) - sum(f) / len(f)
        spread = max(max(s) - min(s), max(f) - min(f))
        print(f"| {name} | {' '.join(f'{v:.1f}' for v in s)} | {' '.join(f'{v:.1f}' for v in f)} | {diff:.1f} | "
              f"{max(s) - min(s):.1f} / {max(f) - min(f):.1f} | {'yes' if diff > 2 * spread else 'no'} | "
              f"{kinds_of(stocks[0][i])} | {kinds_of(flips[0][i])} |")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(sys.argv[2:])
