"""gate(BatchNorm2d(y)) with gate = SE or ECA as one autograd node on the HIP passes of mrla_amd/csrc/bn_gate_nhwc.hip
(functional.bn_gate / functional.CHANNEL_GATE; reference resnet_mrla_light.py:77-81,105-108, modules/se_module.py,
modules/eca_module.py).

The comparison target is the float64 restatement of tests/channel_gate_cases.py.  Bounds:
  fp32        out, dy, running statistics: cases.ACT_TOL.
  bf16 / fp16 operands rounded to the type first, the target computed from the rounded values; out, dy: relmax <= 2^-8 /
              2^-11 (one rounding of the result, half an ulp = 2^-9 / 2^-12 of an element <= that fraction of the maximum,
              doubled for the fp32 accumulation).
  parameter gradients (dgamma, dbeta, ECA's dw, SE's dW1 / dW2), every dtype: the larger of cases.PAR_TOL and 4 x the error
              of the CHANNEL_GATE = False route on the same GPU, the same inputs, against the same float64 values -- the
              gate-weight sums cancel the way dWq / dWk do (cases.QK_TOL's note), so the stock route is the yardstick.
Both errors of every case go to channel_gate_parity.jsonl beside cases.PARITY_LOG (profiles/channel_gate.md quotes them)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests import channel_gate_cases as cg

pytestmark = pytest.mark.gpu

ACT_TOL, PAR_TOL, GOLD_TOL = cases.ACT_TOL, cases.PAR_TOL, cases.GOLD_TOL
_TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_HALF_TOL = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
_LOG = os.path.join(os.path.dirname(os.path.abspath(cases.PARITY_LOG)), "channel_gate_parity.jsonl")
_CL = torch.channels_last


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _log(**rec):
    try:
        os.makedirs(os.path.dirname(_LOG), exist_ok=True)
        with open(_LOG, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    except Exception:
        pass


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-12))


@functools.lru_cache(maxsize=None)
def _split_shape():
    """The smallest 2 x 64 x h x w map whose plane-moment rows outnumber its images (an image split over workgroups)."""
    from mrla_amd import _lib as L
    rows = L.load().mrla_bn_moment_rows
    assert rows(2, 64, 56, 56, L.NHWC) > 2
    for hw in range(1, 56 * 56 + 1):
        for h in range(int(hw ** 0.5), 0, -1):
            if hw % h == 0 and rows(2, 64, h, hw // h, L.NHWC) > 2:
                return (2, 64, h, hw // h)
    raise AssertionError("no split shape")


@functools.lru_cache(maxsize=None)
def _case(shape, gate, dtype, training):
    """Inputs (rounded to the storage type), parameters and the float64 target of one case: computed once, never modified."""
    b, c, h, w = shape
    y, do = cg.inputs(b, c, h, w)
    p = cg.params(c, gate)
    td = _TD[dtype]
    yt, dot = torch.from_numpy(y).to(td), torch.from_numpy(do).to(td)
    want = cg.restate_f64(yt.double().numpy(), dot.double().numpy(), p, gate, training)
    return yt, dot, p, want


def _modules(c, gate, p):
    from mrla_amd import resnet as R
    bn = nn.BatchNorm2d(c, eps=cg.EPS, momentum=cg.MOMENTUM)
    mod = R.se_layer(c, reduction=16) if gate == "se" else R.eca_layer(c, int(gate[3:]))
    net = nn.ModuleDict({"bn": bn, "se" if gate == "se" else "eca": mod})
    missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"bn.num_batches_tracked"}
    return net.cuda()


def _run(shape, gate, dtype, training, on):
    """One forward + backward of functional.bn_gate with CHANNEL_GATE = on -> the arrays restate_f64 names, and the C-ABI
    entries that were called."""
    from mrla_amd import functional as Fm
    yt, dot, p, _ = _case(shape, gate, dtype, training)
    net = _modules(shape[1], gate, p)
    net.train(training)
    bn = net["bn"]
    se, eca = (net["se"], None) if gate == "se" else (None, net["eca"])
    x = yt.cuda().contiguous(memory_format=_CL).requires_grad_(True)
    gup = dot.cuda().contiguous(memory_format=_CL)
    old, Fm.CHANNEL_GATE = Fm.CHANNEL_GATE, on
    try:
        with cg.recorded() as calls:
            with torch.autocast("cuda", dtype=_TD[dtype], enabled=dtype != "f32"):
                out = Fm.bn_gate(x, bn, se=se, eca=eca)
                assert ("_BnGateFn" in type(out.grad_fn).__name__) == on
            out.backward(gup)
            torch.cuda.synchronize()
    finally:
        Fm.CHANNEL_GATE = old
    assert out.dtype == _TD[dtype] and x.grad.dtype == _TD[dtype] and out.is_contiguous(memory_format=_CL)
    res = {"out": out.detach().float().cpu().numpy(), "dx": x.grad.float().cpu().numpy(),
           "new_rm": bn.running_mean.cpu().numpy(), "new_rv": bn.running_var.cpu().numpy()}
    for k, v in net.named_parameters():
        assert v.grad is not None and v.grad.dtype == v.dtype and v.grad.shape == v.shape, k
        res["grad/" + k] = v.grad.float().cpu().numpy()
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    return res, [n for n, _ in calls]


_NEW = ("mrla_bn_gate_pool", "mrla_bn_gate_sums_bwd", "mrla_bn_gate_fwd", "mrla_bn_gate_bwd")


def _check(shape, gate, dtype, training):
    _, _, _, want = _case(shape, gate, dtype, training)
    on, names_on = _run(shape, gate, dtype, training, True)
    off, names_off = _run(shape, gate, dtype, training, False)
    assert all(n in names_on for n in _NEW) and not any(n in names_off for n in _NEW), (names_on, names_off)
    assert ("mrla_eca_gate_fwd" in names_on) == (gate != "se") and ("mrla_eca_gate_bwd" in names_on) == (gate != "se")
    act = ACT_TOL if dtype == "f32" else _HALF_TOL[dtype]
    tag = dict(shape="x".join(map(str, shape)), gate=gate, dtype=dtype, mode="train" if training else "eval")
    for k in ("out", "dx"):
        assert np.isfinite(on[k]).all()
        e_on, e_off = _rel(on[k], want[k]), _rel(off[k], want[k])
        _log(**tag, what=k, hip=e_on, stock=e_off, bound=act)
        print(tag, k, f"hip {e_on:.3e} stock {e_off:.3e} bound {act:.3e}")
        assert e_on <= act, (k, e_on)
    if dtype == "f32":
        for k in ("new_rm", "new_rv"):
            assert _rel(on[k], want[k]) <= ACT_TOL, k
    for k in sorted(want):
        if not k.startswith("grad/"):
            continue
        e_on, e_off = _rel(on[k], want[k]), _rel(off[k], want[k])
        bound = max(PAR_TOL, 4.0 * e_off)
        _log(**tag, what=k, hip=e_on, stock=e_off, bound=bound)
        print(tag, k, f"hip {e_on:.3e} stock {e_off:.3e} bound {bound:.3e}")
        assert e_on <= bound, (k, e_on, e_off)


# 2x64x7x7: odd pixel count (the tail of the pixel loop); 3x128x5x6; 2x256x7x5; 2x192x3x5: a channel count that is no power
# of two (a thread's channels change from vector to vector); 1x64x1x1: eval only (train-mode BatchNorm is degenerate there);
# "split": more moment rows than images.
SHAPES = [(2, 64, 7, 7), (3, 128, 5, 6), (2, 256, 7, 5), (2, 192, 3, 5), (1, 64, 1, 1), "split"]
GATES = ["eca3", "eca5", "eca7", "se"]


def _shape(s):
    if s == "split":
        from mrla_amd import _lib as L
        s = _split_shape()
        assert L.load().mrla_bn_moment_rows(*s, L.NHWC) > s[0]
    return s


def _ids(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


FP32_CASES = [(s, g, t) for s in SHAPES for g in GATES for t in (True, False) if not (t and s == (1, 64, 1, 1))]


@pytest.mark.parametrize("shape,gate,training", FP32_CASES,
                         ids=[f"{_ids(s)}-{g}-{'train' if t else 'eval'}" for s, g, t in FP32_CASES])
def test_fp32_parity(shape, gate, training):
    _check(_shape(shape), gate, "f32", training)


HALF_CASES = [(d,) + c for d in ("bf16", "f16") for c in FP32_CASES]          # the same shapes x gates x modes in each type


@pytest.mark.parametrize("dtype,shape,gate,training", HALF_CASES,
                         ids=[f"{d}-{_ids(s)}-{g}-{'train' if t else 'eval'}" for d, s, g, t in HALF_CASES])
def test_half_parity(dtype, shape, gate, training):
    _check(_shape(shape), gate, dtype, training)


# ------------------------------------------------------------------------------------------------------
# bit-level anchors and fully written outputs, through the C ABI
# ------------------------------------------------------------------------------------------------------
# the last shape: 5 workgroup iterations per workgroup -- the unrolled loop of four and its remainder, and a last workgroup
# of an image that ends short (iterations per workgroup = ceil(b * ceil(h*w*c / (16-byte vectors of 256 lanes)) / 4096))
ANCHOR_SHAPES = [(2, 64, 7, 7), (2, 192, 3, 5), (1, 64, 1, 1), (2, 2048, 3, 3), (3, 256, 31, 17), (4, 256, 184, 184)]


def _coefficients(b, c, gen):
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)        # noqa: E731
    sc, sh = torch.rand((c,), device="cuda", generator=gen) + 0.5, rnd(c) * 0.5
    sc[::7] = 0.0                                       # bn3's zero-initialised scale
    sc[3::11] *= -1.0
    cb = torch.stack([torch.rand((c,), device="cuda", generator=gen) + 0.5, rnd(c) * 0.25, rnd(c) * 0.1], dim=1).contiguous()
    g, q = torch.sigmoid(rnd(b, c)), rnd(b, c) * 0.05
    return sc, sh, cb, g, q


@pytest.mark.parametrize("shape", ANCHOR_SHAPES, ids=_ids)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_apply_passes_anchor_on_the_plain_batchnorm_passes(dtype, shape):
    """g = 1 (and q = 0): mrla_bn_gate_fwd / _bwd are mrla_bn_act_fwd / _bwd(relu = 0) bit for bit.  A general g, q: the
    float64 formula on the same operands.  Every output is pre-filled with NaN."""
    from mrla_amd import _lib as L
    b, c, h, w = shape
    td, dt = _TD[dtype], {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}[dtype]
    assert L.load().mrla_bn_gate_supported(b, c, h, w, dt, L.NHWC) == 1
    gen = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn((b, h * w, c), device="cuda", generator=gen).to(td)                 # NHWC storage
    do = torch.randn((b, h * w, c), device="cuda", generator=gen).to(td)
    sc, sh, cb, g, q = _coefficients(b, c, gen)
    ones, zeros = torch.ones_like(g), torch.zeros_like(q)
    nan = lambda: torch.full_like(y, float("nan"))      # noqa: E731
    dims = (b, c, h, w, dt, L.NHWC, _stream())
    f0, f1, f2, b0, b1, b2 = (nan() for _ in range(6))
    L.call("mrla_bn_act_fwd", _P(y), _P(sc), _P(sh), 0, _P(f0), *dims)
    L.call("mrla_bn_gate_fwd", _P(y), _P(sc), _P(sh), _P(ones), _P(f1), *dims)
    L.call("mrla_bn_gate_fwd", _P(y), _P(sc), _P(sh), _P(g), _P(f2), *dims)
    L.call("mrla_bn_act_bwd", _P(do), _P(y), _P(sc), _P(sh), _P(cb), 0, _P(b0), *dims)
    L.call("mrla_bn_gate_bwd", _P(do), _P(y), _P(cb), _P(ones), _P(zeros), _P(b1), *dims)
    L.call("mrla_bn_gate_bwd", _P(do), _P(y), _P(cb), _P(g), _P(q), _P(b2), *dims)
    torch.cuda.synchronize()
    for t in (f1, f2, b1, b2):
        assert torch.isfinite(t).all()
    assert torch.equal(f1, f0), f"forward: {int((f1 != f0).sum())} of {f0.numel()} elements differ"
    assert torch.equal(b1, b0), f"backward: {int((b1 != b0).sum())} of {b0.numel()} elements differ"
    tol = ACT_TOL if dtype == "f32" else _HALF_TOL[dtype]
    yd, dd, gd, qd = y.double(), do.double(), g.double()[:, None, :], q.double()[:, None, :]
    want_f = gd * (sc.double() * yd + sh.double())
    e, f, hh = cb[:, 0].double(), cb[:, 1].double(), cb[:, 2].double()
    want_b = (e * gd) * dd + f * yd + (hh + e * qd)
    for got, want in ((f2, want_f), (b2, want_b)):
        err = float((got.double() - want).abs().max() / want.abs().max())
        assert err <= tol, err


@pytest.mark.parametrize("shape", [(2, 64, 7, 7), "split"], ids=_ids)
def test_small_kernels_write_every_output_and_agree_with_float64(shape):
    """The [b,c] kernels through the C ABI on NaN-filled outputs: plane sums and pooled means (pivoted and raw rows), the
    ECA gate and its backward, dg and the BatchNorm-backward rows."""
    from mrla_amd import _lib as L
    b, c, h, w = _shape(shape)
    hw, k = h * w, 5
    lib = L.load()
    rows = lib.mrla_bn_moment_rows(b, c, h, w, L.NHWC)
    ns = rows // b
    gen = torch.Generator(device="cuda").manual_seed(9)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)        # noqa: E731
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")          # noqa: E731
    y = (rnd(b, hw, c) * 0.7 + rnd(c) * 2.0).contiguous()
    do = rnd(b, hw, c)
    sc, sh, _, _, _ = _coefficients(b, c, gen)
    mean = y.double().mean((0, 1)).float()
    wk = rnd(k) * 0.8
    st = _stream()
    S64 = y.double().sum(1)
    pooled64 = sc.double() * S64 / hw + sh.double()
    for pivoted in (True, False):
        amom, pivot = nan(rows, c, 2), (nan(c) if pivoted else None)
        S, pooled = nan(b, c), nan(b, c)
        L.call("mrla_bn_plane_moments", _P(y), _P(amom), _P(pivot), b, c, h, w, L.F32, L.NHWC, st)
        L.call("mrla_bn_gate_pool", _P(amom), _P(pivot), _P(sc), _P(sh), _P(S), _P(pooled), b, c, h, w, L.NHWC, st)
        torch.cuda.synchronize()
        assert torch.isfinite(S).all() and torch.isfinite(pooled).all()
        assert float((S.double() - S64).abs().max() / S64.abs().max()) < ACT_TOL
        assert float((pooled.double() - pooled64).abs().max() / pooled64.abs().max()) < ACT_TOL
    g = nan(b, c)
    L.call("mrla_eca_gate_fwd", _P(pooled), _P(wk), k, _P(g), b, c, st)
    p64 = pooled.double().requires_grad_(True)
    w64 = wk.double().requires_grad_(True)
    g64 = torch.sigmoid(torch.nn.functional.conv1d(p64.unsqueeze(1), w64.view(1, 1, k), padding=(k - 1) // 2).squeeze(1))
    arows, dg, q, dwp, tmom = nan(rows, c, 2), nan(b, c), nan(b, c), nan(b + 1, k), nan(b, c, 2)
    L.call("mrla_bn_plane_dmoments", _P(do), _P(y), _P(sc), _P(sh), _P(mean), 0, _P(arows), b, c, h, w, L.F32, L.NHWC, st)
    sums = (_P(arows), _P(S), _P(g))
    bn3 = (_P(sc), _P(sh), _P(mean))
    L.call("mrla_bn_gate_sums_bwd", *sums, None, *bn3, _P(dg), None, b, c, h, w, L.NHWC, st)
    L.call("mrla_eca_gate_bwd", _P(dg), _P(g), _P(pooled), _P(wk), k, _P(q), _P(dwp), _P(dwp[b]), b, c, hw, st)
    L.call("mrla_bn_gate_sums_bwd", *sums, _P(q), *bn3, None, _P(tmom), b, c, h, w, L.NHWC, st)
    torch.cuda.synchronize()
    for t in (g, arows, dg, q, dwp, tmom):
        assert torch.isfinite(t).all()
    assert ns >= 1 and arows.shape[0] == b * ns
    z64 = sc.double() * y.double() + sh.double()
    dg64 = (do.double() * z64).sum(1)
    (g64 * dg64).sum().backward()
    q64 = p64.grad / hw
    dz64 = g64.detach()[:, None, :] * do.double() + q64[:, None, :]
    t64 = torch.stack([dz64.sum(1), (dz64 * (y.double() - mean.double())).sum(1)], dim=2)
    rel = lambda a, b_: float((a.double() - b_).abs().max() / b_.abs().max())          # noqa: E731
    assert rel(g, g64.detach()) < ACT_TOL and rel(dg, dg64) < ACT_TOL and rel(q, q64) < PAR_TOL
    assert rel(dwp[b], w64.grad) < PAR_TOL and rel(tmom, t64) < PAR_TOL
    assert rel(dwp[b], dwp[:b].double().sum(0)) < ACT_TOL                 # the fold of the per-image partials


# ------------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------------
class _forwards_entered:
    """Counts the calls of the eager gate modules' forward methods."""

    def __enter__(self):
        from mrla_amd import resnet as R
        self.n = {"se": 0, "eca": 0}
        self.real = {"se": R.se_layer.forward, "eca": R.eca_layer.forward}

        def wrap(key):
            def forward(mod, x):
                self.n[key] += 1
                return self.real[key](mod, x)
            return forward
        R.se_layer.forward, R.eca_layer.forward = wrap("se"), wrap("eca")
        return self.n

    def __exit__(self, *exc):
        from mrla_amd import resnet as R
        R.se_layer.forward, R.eca_layer.forward = self.real["se"], self.real["eca"]


def _block(seed=3, **kw):
    from mrla_amd import resnet as R
    torch.manual_seed(seed)
    blk = R.MRLA_Bottleneck(64, 16, **kw).cuda()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return blk.to(memory_format=_CL)


def _block_io(dtype, cl=True):
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.relu(torch.randn((2, 64, 8, 8), device="cuda", generator=gen) + 0.3).to(dtype)
    gup = (torch.randn((2, 64, 8, 8), device="cuda", generator=gen) * 0.1).to(dtype)
    return (x.contiguous(memory_format=_CL), gup.contiguous(memory_format=_CL)) if cl else (x.contiguous(), gup.contiguous())


def _block_step(blk, x, gup, on, autocast):
    from mrla_amd import functional as Fm
    old, Fm.CHANNEL_GATE = Fm.CHANNEL_GATE, on
    try:
        blk.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(True)
        with cg.recorded() as calls, _forwards_entered() as entered:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                out = blk(xp)
            out.backward(gup)
            torch.cuda.synchronize()
    finally:
        Fm.CHANNEL_GATE = old
    grads = {k: p.grad.clone() for k, p in blk.named_parameters()}
    return out.detach().clone(), xp.grad.clone(), grads, [n for n, _ in calls], dict(entered)


@pytest.mark.parametrize("kw", [dict(ECA_size=3), dict(SE=True)], ids=["eca", "se"])
def test_block_holds_to_its_route(kw):
    blk = _block(**kw)
    keys = set(blk.state_dict())
    assert ({"eca.conv.weight"} if "ECA_size" in kw else {"se.fc.0.weight", "se.fc.2.weight"}) <= keys
    assert not any(k.startswith(("se.", "eca.")) for k in keys - {"eca.conv.weight", "se.fc.0.weight", "se.fc.2.weight"})
    x, gup = _block_io(torch.bfloat16)
    which = "eca" if "ECA_size" in kw else "se"
    # switch on: the new entries, never the eager forward
    out, dx, grads, names, entered = _block_step(blk, x, gup, True, True)
    assert all(n in names for n in _NEW), names
    assert ("mrla_eca_gate_fwd" in names and "mrla_eca_gate_bwd" in names) == (which == "eca")
    assert entered == {"se": 0, "eca": 0}
    assert torch.isfinite(out.float()).all() and torch.isfinite(dx.float()).all()
    assert all(g is not None and torch.isfinite(g.float()).all() for g in grads.values())
    # switch off: the eager forward, none of the new entries
    _, _, _, names, entered = _block_step(blk, x, gup, False, True)
    assert not any(n.startswith(("mrla_bn_gate", "mrla_eca_gate")) for n in names), names
    assert entered[which] == 1 and entered["se" if which == "eca" else "eca"] == 0
    # an NCHW input: eager, switch on or not
    xn, gn = _block_io(torch.bfloat16, cl=False)
    nchw = _block(**kw).to(memory_format=torch.contiguous_format)
    _, _, _, names, entered = _block_step(nchw, xn, gn, True, True)
    assert not any(n.startswith(("mrla_bn_gate", "mrla_eca_gate")) for n in names), names
    assert entered[which] == 1


def test_both_gates_at_once_stay_eager():
    blk = _block(SE=True, ECA_size=3)
    assert {"eca.conv.weight", "se.fc.0.weight", "se.fc.2.weight"} <= set(blk.state_dict())
    x, gup = _block_io(torch.bfloat16)
    _, _, _, names, entered = _block_step(blk, x, gup, True, True)
    assert not any(n.startswith(("mrla_bn_gate", "mrla_eca_gate")) for n in names), names
    assert entered == {"se": 1, "eca": 1}


def test_basic_block_takes_the_route_too():
    from mrla_amd import resnet as R
    torch.manual_seed(2)
    blk = R.MRLA_BasicBlock(64, 64, ECA_size=3).cuda().to(memory_format=_CL)
    x, gup = _block_io(torch.float32)
    _, _, _, names, entered = _block_step(blk, x, gup, True, False)
    assert all(n in names for n in _NEW) and entered == {"se": 0, "eca": 0}


@pytest.mark.parametrize("kw", [dict(ECA_size=3), dict(SE=True)], ids=["eca", "se"])
def test_block_level_switch_on_against_off(kw):
    """The same fp32 channels_last block, switch on and off: outputs and every parameter gradient differ by no more than two
    switch-off runs differ from each other (MIOpen's 3x3 is not bit-stable: the noise is measured here) plus ACT_TOL /
    PAR_TOL."""
    blk = _block(**kw)
    x, gup = _block_io(torch.float32)
    state = {k: v.clone() for k, v in blk.state_dict().items()}

    def run(on):
        blk.load_state_dict(state)
        return _block_step(blk, x, gup, on, False)
    off1, off2, on = run(False), run(False), run(True)
    assert all(n in on[3] for n in _NEW) and on[4] == {"se": 0, "eca": 0}
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-12))    # noqa: E731
    for i, what in ((0, "out"), (1, "dx")):
        noise, err = rel(off2[i], off1[i]), rel(on[i], off1[i])
        print(what, f"on/off {err:.3e} off/off {noise:.3e}")
        assert err <= noise + ACT_TOL, (what, err, noise)
    assert on[2].keys() == off1[2].keys() and len(on[2]) >= 15
    for k in on[2]:
        noise, err = rel(off2[2][k], off1[2][k]), rel(on[2][k], off1[2][k])
        print(k, f"on/off {err:.3e} off/off {noise:.3e}")
        assert err <= noise + PAR_TOL, (k, err, noise)


def test_gradient_at_an_unaligned_address():
    """A channels_last gradient whose storage starts 4 bytes into an allocation: the backward copies it to an aligned
    buffer instead of failing on the 16-byte check of the passes; same values."""
    from mrla_amd import functional as Fm
    shape, gate = (2, 64, 7, 7), "eca3"
    yt, dot, p, _ = _case(shape, gate, "f32", True)
    b, c, h, w = shape
    aligned = dot.cuda().contiguous(memory_format=_CL)
    base = torch.empty(aligned.numel() + 1, device="cuda")
    odd = base[1:].view(b, h, w, c).permute(0, 3, 1, 2)
    odd.copy_(aligned)
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous(memory_format=_CL)
    got = []
    for gup in (aligned, odd):
        net = _modules(c, gate, p).train()
        x = yt.cuda().contiguous(memory_format=_CL).requires_grad_(True)
        out = Fm.bn_gate(x, net["bn"], eca=net["eca"])
        assert "_BnGateFn" in type(out.grad_fn).__name__
        out.backward(gup)
        torch.cuda.synchronize()
        got.append((x.grad.clone(), net["eca"].conv.weight.grad.clone(), net["bn"].weight.grad.clone()))
    for u, v in zip(*got):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------
# the reference's own float32 run
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cg.GOLDEN_CASES, ids=[c[0] for c in cg.GOLDEN_CASES])
def test_golden(case):
    """The reference's own float32 run.  out / dx are compared on the strided samples the fixture stores (every 2nd element
    of the two small cases, every 16th of 2x256x7x5: channel_gate_cases.strides_of, the fixture stays under 200 KB); the
    float64 parity tests above compare the same tensors in full."""
    name, b, c, h, w, gate = case
    G = cases.golden("channel_gate")
    shape = (b, c, h, w)
    _, st = cg.strides_of(b * c * h * w)
    on, names = _run(shape, gate, "f32", True, True)
    off, _ = _run(shape, gate, "f32", True, False)
    assert all(n in names for n in _NEW)
    for k in ("out", "dx"):
        assert cases.relmax(cg.sample(on[k], st), G[f"{name}/f32/{k}"]) < GOLD_TOL, k
    for k in cg.gate_keys(gate):
        assert cases.relmax(on["grad/" + k], G[f"{name}/f32/grad/{k}"]) < GOLD_TOL, k
    for k in ("grad/bn.weight", "grad/bn.bias"):         # the two-sided rule, against the reference's float64 run
        want = G[f"{name}/f64/{k}"]
        e_on, e_off = _rel(on[k], want), _rel(off[k], want)
        assert e_on <= max(PAR_TOL, 4.0 * e_off), (k, e_on, e_off)


# ------------------------------------------------------------------------------------------------------
# graph capture
# ------------------------------------------------------------------------------------------------------
def test_captured_forward_backward_replays_equal_eager():
    from mrla_amd import functional as Fm
    shape, gate = (2, 64, 7, 7), "eca3"
    yt, dot, p, _ = _case(shape, gate, "f32", True)
    net = _modules(64, gate, p).train()
    bn, eca = net["bn"], net["eca"]
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x0 = yt.cuda().contiguous(memory_format=_CL)
    gup = dot.cuda().contiguous(memory_format=_CL)

    def run(x):
        out = Fm.bn_gate(x, bn, eca=eca)
        assert "_BnGateFn" in type(out.grad_fn).__name__
        out.backward(gup)
        return out

    def results(x, out):
        return [x.grad, bn.weight.grad, bn.bias.grad, eca.conv.weight.grad, bn.running_mean, bn.running_var, out.detach()]

    def eager():
        # on a leaf of its own, and only clones leave: a result that kept this step's autograd graph -- and with it the
        # parameters' AccumulateGrad nodes, created on this stream -- alive into the capture makes capture_end crash
        # (benchkit/common.py, make_step)
        xe = x0.clone().requires_grad_(True)
        out = run(xe)
        torch.cuda.synchronize()
        return [t.clone() for t in results(xe, out)]
    want = eager()
    net.zero_grad(set_to_none=True)
    net.load_state_dict(state)
    xs = x0.clone().requires_grad_(True)

    def step():
        return run(xs)

    def grads():
        return results(xs, out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    net.zero_grad(set_to_none=True)
    net.load_state_dict(state)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        net.load_state_dict(state)
        graph.replay()
        torch.cuda.synchronize()
        for name, u, v in zip(("dx", "dgamma", "dbeta", "dw", "rm", "rv", "out"), grads(), want):
            assert torch.equal(u, v), f"{name}: {int((u != v).sum())} of {u.numel()} elements differ from the eager run"
