#!/usr/bin/env python
"""Times gate(bn(y)) forward + backward with functional.CHANNEL_GATE on and off, alternating in one process.

    timeout 900 python scripts/time_channel_gate.py [--out channel_gate_timing.json]

Shapes: the four stage shapes of ResNet-50 at batch 256 and one detection map, bf16 channels_last under autocast, once with
ECA and once with SE.  HIP events around 20 iterations after 5 warm-ups, three rounds per route (on, off, on, off, ...);
the table holds the median round.  N = bytes of one activation tensor; the HIP route is built to move 3N + 5N."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7), (2, 256, 200, 336)]


def time_route(Fm, on, x, gup, bn, se, eca, iters, warmup, autocast=True):
    Fm.CHANNEL_GATE = on
    xp = x.detach().requires_grad_(True)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = Fm.bn_gate(xp, bn, se=se, eca=eca)
        out.backward(gup)
        xp.grad = None
    for _ in range(warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16",
                    help="fp32: no autocast -- at c = 2048 (and any c that does not divide 1024) the apply kernel's lanes "
                         "change channels from vector to vector")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_channel_gate.py: no GPU visible; a time is a GPU measurement")
    from mrla_amd import functional as Fm
    from mrla_amd import resnet as R
    rows = []
    for gate in ("eca", "se"):
        for b, c, h, w in SHAPES:
            torch.manual_seed(0)
            bn = nn.BatchNorm2d(c).cuda()
            se = R.se_layer(c).cuda() if gate == "se" else None
            eca = R.eca_layer(c).cuda() if gate == "eca" else None
            td = torch.bfloat16 if a.dtype == "bf16" else torch.float32
            x = torch.randn((b, c, h, w), device="cuda").to(td).contiguous(memory_format=torch.channels_last)
            gup = torch.randn((b, c, h, w), device="cuda").to(td).contiguous(memory_format=torch.channels_last)
            t = {True: [], False: []}
            for _ in range(a.rounds):
                for on in (True, False):
                    t[on].append(time_route(Fm, on, x, gup, bn, se, eca, a.iters, a.warmup, a.dtype == "bf16"))
            Fm.CHANNEL_GATE = True
            n_bytes = x.numel() * x.element_size()
            on_ms, off_ms = statistics.median(t[True]), statistics.median(t[False])
            rows.append(dict(gate=gate, shape=[b, c, h, w], n_mb=n_bytes / 1e6, hip_ms=on_ms, stock_ms=off_ms,
                             hip_all=t[True], stock_all=t[False], hip_tb_s=8 * n_bytes / on_ms / 1e9))
            print(f"{gate:4s} {b}x{c}x{h}x{w}: HIP {on_ms:.3f} ms (8N at {rows[-1]['hip_tb_s']:.2f} TB/s)  stock {off_ms:.3f} ms  "
                  f"x{off_ms / on_ms:.2f}", flush=True)
            del x, gup
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    print("| gate | shape | N (MB) | HIP ms | stock ms | stock / HIP |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['gate']} | {'x'.join(map(str, r['shape']))} | {r['n_mb']:.1f} | {r['hip_ms']:.3f} | {r['stock_ms']:.3f} | "
              f"{r['stock_ms'] / r['hip_ms']:.2f} |")


if __name__ == "__main__":
    main()
