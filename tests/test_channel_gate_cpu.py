"""Host side of the BatchNorm + channel attention passes (mrla_amd/csrc/bn_gate_nhwc.hip): argument validation of every new
C-ABI entry (validation comes before any launch: needs the built library, not a GPU), and the eager se_layer / eca_layer
route and the tests' own float64 restatement against what the reference's modules computed
(tests/golden/channel_gate.npz, scripts/make_channel_gate_golden.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cases
from tests import channel_gate_cases as cg

P = ctypes.c_void_p
one, odd = P(16), P(24)             # an aligned and a misaligned non-null "pointer": nothing is launched in these tests


def _lib():
    from mrla_amd import _lib as L
    return L, L.load()


def test_symbols_and_supported_answers():
    L, lib = _lib()
    for name in ("mrla_bn_gate_supported", "mrla_bn_gate_pool", "mrla_eca_gate_fwd", "mrla_eca_gate_bwd",
                 "mrla_bn_gate_sums_bwd", "mrla_bn_gate_fwd", "mrla_bn_gate_bwd"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.mrla_abi_version() == 5
    sup = lib.mrla_bn_gate_supported
    for dt in (L.F32, L.BF16, L.F16):
        # the four stage shapes of ResNet-50, a detection map, the BasicBlock widths, the smallest map
        for b, c, h, w in ((256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7), (2, 256, 200, 336),
                           (2, 64, 7, 7), (3, 128, 5, 6), (2, 192, 3, 5), (1, 64, 1, 1)):
            assert sup(b, c, h, w, dt, L.NHWC) == 1, (b, c, h, w, dt)
            assert sup(b, c, h, w, dt, L.NCHW) == L.EUNSUPPORTED
        assert sup(0, 64, 7, 7, dt, L.NHWC) == L.EINVAL and sup(2, 64, 0, 7, dt, L.NHWC) == L.EINVAL
        assert sup(2, 64, 7, 7, dt, 7) == L.EINVAL
    # whole 16-byte channel vectors: 4 floats, 8 halves
    assert sup(2, 36, 7, 7, L.F32, L.NHWC) == 1 and sup(2, 36, 7, 7, L.BF16, L.NHWC) == L.EUNSUPPORTED
    assert sup(2, 66, 7, 7, L.F32, L.NHWC) == L.EUNSUPPORTED and sup(2, 66, 7, 7, L.F16, L.NHWC) == L.EUNSUPPORTED
    assert sup(2, 64, 7, 7, 9, L.NHWC) == L.EINVAL
    # the image index is a grid dimension
    assert sup(65535, 64, 1, 1, L.BF16, L.NHWC) == 1 and sup(65536, 64, 1, 1, L.BF16, L.NHWC) == L.EUNSUPPORTED


def test_pool_validation():
    L, lib = _lib()

    def call(amom=one, sc=one, sh=one, S=one, pooled=one, b=2, c=64, h=7, w=7, layout=L.NHWC):
        return lib.mrla_bn_gate_pool(amom, None, sc, sh, S, pooled, b, c, h, w, layout, None)
    for k in ("amom", "sc", "sh", "S", "pooled"):
        assert call(**{k: None}) == L.EINVAL, k
    assert call(b=0) == L.EINVAL and call(c=0) == L.EINVAL and call(h=0) == L.EINVAL and call(w=-1) == L.EINVAL
    assert call(layout=L.NCHW) == L.EUNSUPPORTED and call(layout=5) == L.EINVAL
    assert call(h=1 << 16, w=1 << 16) == L.EUNSUPPORTED                              # h*w as an int


def test_eca_validation():
    L, lib = _lib()

    def fwd(pooled=one, w=one, k=3, g=one, b=2, c=64):
        return lib.mrla_eca_gate_fwd(pooled, w, k, g, b, c, None)

    def bwd(dg=one, g=one, pooled=one, w=one, k=3, q=one, part=one, dw=one, b=2, c=64, hw=49):
        return lib.mrla_eca_gate_bwd(dg, g, pooled, w, k, q, part, dw, b, c, hw, None)
    for k in ("pooled", "w", "g"):
        assert fwd(**{k: None}) == L.EINVAL, k
    for k in ("dg", "g", "pooled", "w", "q", "part", "dw"):
        assert bwd(**{k: None}) == L.EINVAL, k
    for f in (fwd, bwd):
        assert f(k=2) == L.EINVAL and f(k=4) == L.EINVAL and f(k=0) == L.EINVAL and f(k=-3) == L.EINVAL      # even / no taps
        assert f(b=0) == L.EINVAL and f(c=0) == L.EINVAL
    assert bwd(hw=0) == L.EINVAL
    assert bwd(b=1 << 20, c=1 << 12) == L.EUNSUPPORTED and fwd(b=1 << 20, c=1 << 12) == L.EUNSUPPORTED   # b*c as an int
    assert fwd(c=1 << 20) == L.EUNSUPPORTED and bwd(c=1 << 20) == L.EUNSUPPORTED       # the padded rows live in LDS


def test_sums_validation():
    L, lib = _lib()

    def call(arows=one, S=one, g=one, q=one, sc=one, sh=one, mean=one, dg=one, tmom=one, b=2, c=64, h=7, w=7, layout=L.NHWC):
        return lib.mrla_bn_gate_sums_bwd(arows, S, g, q, sc, sh, mean, dg, tmom, b, c, h, w, layout, None)
    for k in ("arows", "sc", "sh", "mean"):
        assert call(**{k: None}) == L.EINVAL, k
    assert call(q=None, dg=None) == L.EINVAL                                          # first form: dg is the output
    for k in ("S", "g", "tmom"):                                                        # second form: tmom from S, g, q
        assert call(**{k: None}) == L.EINVAL, k
    assert call(arows=odd) == L.EINVAL
    assert call(b=0) == L.EINVAL and call(c=-1) == L.EINVAL and call(h=0) == L.EINVAL
    assert call(layout=L.NCHW) == L.EUNSUPPORTED and call(q=None, layout=L.NCHW) == L.EUNSUPPORTED
    assert call(h=1 << 16, w=1 << 16) == L.EUNSUPPORTED


@pytest.mark.parametrize("dt", ["F32", "BF16", "F16"])
def test_apply_validation(dt):
    L, lib = _lib()
    dt = getattr(L, dt)

    def fwd(y=one, sc=one, sh=one, g=one, out=P(32), b=2, c=64, h=7, w=7, dtype=dt, layout=L.NHWC):
        return lib.mrla_bn_gate_fwd(y, sc, sh, g, out, b, c, h, w, dtype, layout, None)

    def bwd(do=one, y=one, cb=one, g=one, q=one, dy=P(32), b=2, c=64, h=7, w=7, dtype=dt, layout=L.NHWC):
        return lib.mrla_bn_gate_bwd(do, y, cb, g, q, dy, b, c, h, w, dtype, layout, None)
    for k in ("y", "sc", "sh", "g", "out"):
        assert fwd(**{k: None}) == L.EINVAL and fwd(**{k: odd}) == L.EINVAL, k          # null / not 16-byte aligned
    for k in ("do", "y", "cb", "g", "q", "dy"):
        assert bwd(**{k: None}) == L.EINVAL and bwd(**{k: odd}) == L.EINVAL, k
    for f in (fwd, bwd):
        assert f(b=0) == L.EINVAL and f(c=0) == L.EINVAL and f(h=0) == L.EINVAL and f(w=0) == L.EINVAL     # m = 0
        assert f(dtype=3) == L.EINVAL
        assert f(layout=L.NCHW) == L.EUNSUPPORTED and f(layout=4) == L.EINVAL
        assert f(c=60 if dt != L.F32 else 62) == L.EUNSUPPORTED                        # not whole 16-byte vectors


def _eager(name, b, c, h, w, gate, dtype):
    """The project's eager modules (the CHANNEL_GATE = False route on a CPU tensor) on a golden case."""
    from mrla_amd import resnet as R
    y, do = cg.inputs(b, c, h, w)
    p = cg.params(c, gate)
    bn = nn.BatchNorm2d(c, eps=cg.EPS, momentum=cg.MOMENTUM)
    mod = R.se_layer(c, reduction=16) if gate == "se" else R.eca_layer(c, int(gate[3:]))
    net = nn.ModuleDict({"bn": bn, "se" if gate == "se" else "eca": mod}).to(dtype)
    assert set(cg.gate_keys(gate)) <= set(net.state_dict())                             # the reference's key names
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in p.items()}, strict=False)
    net.train()
    x = torch.from_numpy(y).to(dtype).requires_grad_(True)
    out = mod(bn(x))
    (out * torch.from_numpy(do).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "dx": x.grad.numpy(), "new_rm": bn.running_mean.numpy(), "new_rv": bn.running_var.numpy()}
    res.update({"grad/" + k: v.grad.numpy() for k, v in net.named_parameters()})
    return res


@pytest.mark.parametrize("case", cg.GOLDEN_CASES, ids=[c[0] for c in cg.GOLDEN_CASES])
def test_golden_pins_inputs_eager_route_and_restatement(case):
    name, b, c, h, w, gate = case
    G = cases.golden("channel_gate")
    y, do = cg.inputs(b, c, h, w)
    ist, st = cg.strides_of(y.size)
    ik = cg.input_key(b, c, h, w)
    assert np.array_equal(G[ik + "/x"], cg.sample(y, ist)) and np.array_equal(G[ik + "/do"], cg.sample(do, ist))
    for k, v in cg.params(c, gate).items():
        assert np.array_equal(G[f"{name}/{k}"], v), k
    keys = ["out", "dx", "new_rm", "new_rv", "grad/bn.weight", "grad/bn.bias"] + ["grad/" + k for k in cg.gate_keys(gate)]

    def sub(k, v, stride):
        return cg.sample(v, stride) if k in ("out", "dx") else v
    # float64: the eager modules and the restatement both reproduce the reference's own double-precision run
    e64, r64 = _eager(*case, torch.float64), cg.restate_f64(y, do, cg.params(c, gate), gate, True)
    for k in keys:
        want = G[f"{name}/f64/{k}"]
        assert cases.relmax(sub(k, e64[k], cg.F64_STRIDE), want) < 1e-12, k
        assert cases.relmax(sub(k, r64[k], cg.F64_STRIDE), want) < 1e-12, k
    # float32: the eager route against the reference's float32 run
    e32 = _eager(*case, torch.float32)
    for k in keys:
        assert cases.relmax(sub(k, e32[k], st), G[f"{name}/f32/{k}"]) < cases.GOLD_TOL, k


def test_fixture_is_small_and_holds_arrays_only():
    import os
    path = os.path.join(cases.GOLDEN, "channel_gate.npz")
    assert os.path.getsize(path) < 200 * 1024
    with np.load(path, allow_pickle=False) as G:
        for k in G.files:
            assert G[k].dtype in (np.float32, np.float64), k


def test_switch_exists_and_defaults_on():
    from mrla_amd import functional as Fm
    assert Fm.CHANNEL_GATE is True
    assert callable(Fm.bn_gate) and issubclass(Fm._BnGateFn, torch.autograd.Function)


def test_cpu_tensors_take_the_eager_route():
    """A CPU block with a gate still runs (the eager modules), as it did before the HIP node existed."""
    from mrla_amd import functional as Fm
    from mrla_amd import resnet as R
    torch.manual_seed(0)
    bn, eca, se = nn.BatchNorm2d(64), R.eca_layer(64, 3), R.se_layer(64)
    x = torch.randn(2, 64, 5, 5)
    for kw in (dict(eca=eca), dict(se=se), dict(se=se, eca=eca)):
        bn2 = nn.BatchNorm2d(64)
        want = bn2(x)
        for m in (kw.get("se"), kw.get("eca")):
            want = m(want) if m is not None else want
        bn.reset_running_stats()
        got = Fm.bn_gate(x, bn, **kw)
        assert torch.equal(got, want)
