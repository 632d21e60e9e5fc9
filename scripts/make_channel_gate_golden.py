#!/usr/bin/env python
"""Writes tests/golden/channel_gate.npz: what the REFERENCE's own se_layer / eca_layer compute behind a train-mode
nn.BatchNorm2d, in float64 and in float32, on the deterministic inputs of tests/channel_gate_cases.py.

    python scripts/make_channel_gate_golden.py --reference /path/to/the/reference/checkout

The reference's modules/eca_module.py and modules/se_module.py are imported where they lie (they need torch only); nothing
of them is copied.  The file holds arrays only: inputs, parameters, out, dx, every parameter gradient and the updated
running statistics.  To keep the file small, out / dx (every float64 one; the float32 ones at channel_gate_cases.strides_of)
and the inputs of the large case are stored as strided samples of the NCHW-flat tensor: the tests regenerate the inputs
from their seed, and the stored values pin the generator."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import channel_gate_cases as cg  # noqa: E402


def _import(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref_eca, ref_se, y, do, p, gate, dtype):
    b, c, h, w = y.shape
    bn = nn.BatchNorm2d(c, eps=cg.EPS, momentum=cg.MOMENTUM)
    mod = ref_se.se_layer(c, reduction=16) if gate == "se" else ref_eca.eca_layer(c, int(gate[3:]))
    net = nn.ModuleDict({"bn": bn, "se" if gate == "se" else "eca": mod}).to(dtype)
    sd = net.state_dict()
    for k, v in p.items():
        assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
        sd[k].copy_(torch.from_numpy(v).to(dtype))
    net.train()
    x = torch.from_numpy(y).to(dtype).requires_grad_(True)
    out = mod(bn(x))
    (out * torch.from_numpy(do).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "dx": x.grad.numpy(), "new_rm": bn.running_mean.numpy(), "new_rv": bn.running_var.numpy()}
    for k, v in net.named_parameters():
        res["grad/" + k] = v.grad.numpy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MRLA_REFERENCE"), required="MRLA_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "channel_gate.npz"))
    a = ap.parse_args()
    mods = os.path.join(a.reference, "resnet", "models", "modules")
    ref_eca, ref_se = _import(os.path.join(mods, "eca_module.py"), "ref_eca_module"), _import(os.path.join(mods, "se_module.py"), "ref_se_module")
    torch.manual_seed(0)
    arrays = {}
    for name, b, c, h, w, gate in cg.GOLDEN_CASES:
        y, do = cg.inputs(b, c, h, w)
        p = cg.params(c, gate)
        ist, st = cg.strides_of(y.size)
        ik = cg.input_key(b, c, h, w)
        arrays[ik + "/x"], arrays[ik + "/do"] = cg.sample(y, ist), cg.sample(do, ist)
        for k, v in p.items():
            arrays[f"{name}/{k}"] = v
        for tag, dtype, stride in (("f64", torch.float64, cg.F64_STRIDE), ("f32", torch.float32, st)):
            res = run(ref_eca, ref_se, y, do, p, gate, dtype)
            for k, v in res.items():
                arrays[f"{name}/{tag}/{k}"] = cg.sample(v, stride) if k in ("out", "dx") else v
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
