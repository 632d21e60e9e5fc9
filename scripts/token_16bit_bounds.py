#!/usr/bin/env python
"""CPU only.  Measures what float32 arithmetic costs the 16-bit fused MRLA-base token module: the rounding reference of
oracle/token_base_storage.py (V_t, dV_t, out and dx rounded to the storage type where the kernels store them) is run in float64
and again in float32 on the cases of tests/test_token_base_geometry_gpu.py, and the worst deviation per tensor kind is written to
profiles/token_16bit_bounds.md.  The test's bounds are 4 x these figures (never below one spacing of the storage type); nothing
here touches the HIP kernels.

    python scripts/token_16bit_bounds.py            # prints the table, rewrites profiles/token_16bit_bounds.md
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_token_base_geometry_gpu as T  # noqa: E402

KINDS = ("dx", "normx.weight", "normx.bias", "mrla.Wq.weight", "mrla.Wk.weight", "mrla.Wv.weight")


def measure(sname):
    """kind -> (worst measure, case, layer); plus the worst `out` error over its derived bound and the share of V_t / out / dx
    elements on which the two arithmetic types round to different storage values."""
    u = T.ULP[sname]
    worst = {k: (0.0, None, None) for k in KINDS}
    out_worst, flips = 0.0, {"V": [0, 0], "out": [0, 0], "dx": [0, 0]}
    np_ = lambda a: a.detach().double().numpy()  # noqa: E731
    for case in T.STORAGE_CASES:
        f64 = T.reference_chain(case, sname, torch.float64)
        f32 = T.reference_chain(case, sname, torch.float32)
        for t in range(case[3]):
            vals = {"dx": T.dx_measure(np_(f32[1][t].grad), np_(f64[1][t].grad))}
            w64 = dict(f64[0][t].named_parameters())
            for pn, pv in f32[0][t].named_parameters():
                vals[pn] = T.par_measure(np_(pv.grad), np_(w64[pn].grad))
            for k, v in vals.items():
                if v > worst[k][0]:
                    worst[k] = (float(v), T.case_id(case), t)
            out_worst = max(out_worst, float(T.out_excess(np_(f32[2][t]), np_(f64[2][t]), float(f64[3][t].abs().max()), u)))
            for name, a, b in (("V", f32[3][t][:, -1], f64[3][t][:, -1]), ("out", f32[2][t], f64[2][t]),
                               ("dx", f32[1][t].grad, f64[1][t].grad)):
                flips[name][0] += int((a.double() != b.double()).sum())
                flips[name][1] += a.numel()
    return worst, out_worst, {k: n / d for k, (n, d) in flips.items()}


def main():
    lines = ["# 16-bit fused MRLA-base token module: what float32 arithmetic costs", "",
             "Written by `scripts/token_16bit_bounds.py` (CPU only; no HIP kernel is involved).  The rounding reference of",
             "`oracle/token_base_storage.py` rounds V_t as it enters the history, the gradient arriving at V_t (what",
             "`mrla_base_dv_combine` stores), and out and dx once at the end.  It is run in float64 (the reference of",
             "`tests/test_token_base_geometry_gpu.py`) and in float32 with the same rounding points; the table holds the worst",
             "deviation of the float32 run from the float64 run over the cases " +
             ", ".join(T.case_id(c) for c in T.STORAGE_CASES) + " and all their layers.", "",
             "Measures: dx -- worst element of `|a - r| / (|r| + 0.05 max|r|)` (the measure of `tests/test_base_gpu.py::"
             "assert_mostly_close`); parameter gradients -- `max|a - r| / max|r|`.  Bound of the test = max(4 x measured, u),",
             "u = 2^-7 (bf16) / 2^-10 (fp16): the factor covers another float32 summation order in the kernels.  The emulation has",
             "no element beyond its own worst, so the test allows no outliers.", ""]
    table = {}
    for sname in T.STORAGE:
        worst, out_worst, flips = measure(sname)
        table[sname] = worst
        u = T.ULP[sname]
        lines += [f"## {sname} (u = {u:.3e})", "", "| tensor | measured | at | bound |", "|---|---|---|---|"]
        for k in KINDS:
            v, cid, t = worst[k]
            lines.append(f"| {k} | {v:.3e} | {cid}, layer {t} | {max(4 * v, u):.3e} |")
        lines += ["", f"`out` of the float32 run against the derived bound `u|r| + u max|V| + ACT_TOL max|r|`: worst element at "
                  f"{out_worst:.3f} of the bound.", "",
                  "Share of elements the two runs round to different storage values: " +
                  ", ".join(f"{k} {v:.2e}" for k, v in flips.items()) + ".", ""]
    text = "\n".join(lines)
    print(text)
    print("MEASURED = {")
    for sname, worst in table.items():
        print(f'    "{sname}": {{' + ", ".join(f'"{k}": {worst[k][0]:.3e}' for k in KINDS) + "},")
    print("}")
    with open(os.path.join(ROOT, "profiles", "token_16bit_bounds.md"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
