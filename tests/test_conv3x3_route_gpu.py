"""GPU: the opt-in route of the 3x3 weight gradient in the Python layer (functional.conv3x3 under mrla_amd.conv3x3_wgrad()).

  * conv3x3(x, conv) with the switch on against the stock module: out and dX come from the same aten calls (within 2 ulps of
    the 16-bit type of the tensor's largest magnitude -- equality is not required of the stock kernels), conv.weight.grad is
    fp32 [n, c, 3, 3], inside the fp32 summation bound of tests/test_conv3x3_wgrad_gpu.py against float64, bit-equal to the
    direct C-ABI call on the same x, dy, and bit-equal on a second backward;
  * launch counts, by wrapping functional._call: once per backward where it applies, never with the switch off or for an
    excluded configuration, whose result is conv(x)'s;
  * whole models, one step with the switch off and on: the same loss, every 3x3 weight gradient within the 2 % relative L2 that
    tests/test_block_bf16_gpu.py asks of parameter gradients, all finite;
  * a captured training step at batch 16 -- where the stock weight gradient is wrong from the second replay on -- passes
    graphed_step's self-check with the switch on."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def _pair(c, n, s):
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(c, n, 3, stride=s, padding=1, bias=False).cuda().to(memory_format=CL)
    return conv, copy.deepcopy(conv)


def _dw64(x, dy, s):
    n, c = dy.shape[1], x.shape[1]
    w = torch.zeros((n, c, 3, 3), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, w, stride=s, padding=1), w, dy)
    return g


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 7, 7, 1), (2, 128, 128, 9, 6, 2)], ids=lambda s: "x".join(map(str, s)))
def test_the_route_against_the_stock_module(shape, dtype):
    import mrla_amd
    from mrla_amd import _lib as L, functional as Fm
    b, c, n, h, w, s = shape
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    stock, ours = _pair(c, n, s)
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn((b, c, h, w), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    dy = torch.randn((b, n, ho, wo), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    xs, xo = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        ys = stock(xs)
        assert Fm.conv3x3_applies(ours, xo)
        with mrla_amd.conv3x3_wgrad():
            yo = Fm.conv3x3(xo, ours)
    assert type(yo.grad_fn).__name__.startswith("_Conv3x3Fn") and yo.dtype == dtype and yo.shape == ys.shape
    ys.backward(dy)
    yo.backward(dy, retain_graph=True)
    for name, got, want in (("out", yo, ys), ("dx", xo.grad, xs.grad)):
        err = float((got.double() - want.double()).abs().max())
        assert err <= 2 * ULP[dtype] * float(want.double().abs().max()), (name, err)
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == (n, c, 3, 3) and gw.stride() == ours.weight.stride()
    # the fp32 summation bound against float64 (tests/test_conv3x3_wgrad_gpu.py, item 2)
    x64, dy64 = x0.double().cpu(), dy.double().cpu()
    want64, a = _dw64(x64, dy64, s), _dw64(x64.abs(), dy64.abs(), s)
    err = (gw.double().cpu() - want64).abs()
    assert bool((err <= (b * ho * wo + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max())
    # ... bit-equal to the C ABI on the same x, dy
    rows = L.load().mrla_conv3x3_wgrad_rows(b, c, n, h, w, s, Fm._DT[dtype])
    part = torch.empty((rows, n, 9, c), dtype=torch.float32, device="cuda")
    direct = torch.empty((n, c, 3, 3), dtype=torch.float32, device="cuda", memory_format=CL)
    L.call("mrla_conv3x3_wgrad", dy.data_ptr(), x0.data_ptr(), part.data_ptr(), direct.data_ptr(), b, c, n, h, w, s, Fm._DT[dtype],
           L.F32, Fm._stream())
    assert torch.equal(gw.view(torch.int32), direct.view(torch.int32))
    # ... and on a second backward
    first = gw.clone()
    ours.weight.grad = None
    yo.backward(dy)
    assert torch.equal(ours.weight.grad.view(torch.int32), first.view(torch.int32))


class _Counter:
    """functional._call with the launches of one entry point counted; the product code is not changed."""

    def __init__(self, monkeypatch, name="mrla_conv3x3_wgrad"):
        from mrla_amd import functional as Fm
        self.n, inner = 0, Fm._call

        def counted(label, *args, **kw):
            self.n += (kw.get("entry") or label) == name
            return inner(label, *args, **kw)
        monkeypatch.setattr(Fm, "_call", counted)


def test_one_launch_per_backward_where_it_applies_and_none_elsewhere(monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).cuda().bfloat16().to(memory_format=CL)
    x = torch.randn(2, 64, 6, 6, device="cuda").bfloat16().contiguous(memory_format=CL)
    with mrla_amd.conv3x3_wgrad():
        for i in range(1, 4):                            # eligible, switch on: once per backward
            Fm.conv3x3(x, conv).float().sum().backward()
            assert count.n == i
    count.n = 0
    y = Fm.conv3x3(x, conv)                              # switch off: the module itself
    assert torch.equal(y, conv(x)) and not type(y.grad_fn).__name__.startswith("_Conv3x3Fn")
    y.float().sum().backward()
    assert count.n == 0
    with mrla_amd.conv3x3_wgrad():
        with torch.no_grad():
            assert torch.equal(Fm.conv3x3(x, conv), conv(x))
        for name, c, make in excluded_configurations():
            xe = make("cuda")
            c = c.cuda().to(xe.dtype).to(memory_format=CL)
            assert not Fm.conv3x3_applies(c, xe), name
            ye = Fm.conv3x3(xe, c)
            assert torch.equal(ye, c(xe)), name
            if ye.requires_grad:
                ye.float().sum().backward()
    assert count.n == 0


def _model_step(arch, on):
    import contextlib
    import io
    import mrla_amd
    from mrla_amd import models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(models, arch)(drop_path=0.0).cuda().to(memory_format=CL).train()
    with torch.no_grad():          # the blocks' last BatchNorm starts at weight 0: every 3x3 weight gradient would be exactly 0
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, 3, 64, 64, device="cuda", generator=g).contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (8,), device="cuda", generator=g)
    with mrla_amd.conv3x3_wgrad(on), torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(net(x), y)
        loss.backward()
    grads = {name + ".weight": m.weight.grad.double().cpu() for name, m in net.named_modules()
             if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1}     # (not the MRLA depthwise ones)
    return float(loss), grads


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_a_model_step_with_the_switch_on_matches_the_step_with_it_off(arch, monkeypatch):
    """One step each with the switch off and on, same seed: the same loss within 2 bf16 ulps, every 3x3 weight gradient within the
    2 % relative L2 of tests/test_block_bf16_gpu.py, all finite, one launch per 3x3 convolution.

    Both steps run with torch.backends.cudnn.deterministic: an A/B comparison needs a stock side that agrees with itself, and at
    batch 8 and 64 x 64 images the stock library's default solvers do not -- with identical input the output of the stock 3x3
    FORWARD convolution (first at layer2.0.conv2) differs from run to run by 1e-3, the train-mode BatchNorms over 32 samples
    per channel amplify that, and two steps with the switch OFF differ by 0.8 .. 27 % in these gradients (measured on MI355X;
    profiles/conv3x3_wgrad.md section 6).  With the deterministic solvers the stock step is bit-equal from run to run and on
    against off measures 1.7e-03 for every convolution of both models: the bf16 rounding of the stock gradient."""
    count = _Counter(monkeypatch)
    was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        loss0, g0 = _model_step(arch, False)
        assert count.n == 0
        loss1, g1 = _model_step(arch, True)
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = was
    print(arch, f"losses off {loss0!r} on {loss1!r}")
    assert count.n == len(g1) > 0                        # every 3x3 convolution of these models is eligible at this size
    ulp = 2.0 ** (torch.tensor(abs(loss0)).log2().floor().item() - 7)
    assert abs(loss1 - loss0) <= 2 * ulp, (loss0, loss1)
    errs = {}
    for name, a in g0.items():
        b = g1[name]
        assert bool(torch.isfinite(b).all()), name
        assert float(a.norm()) > 0 and float(b.norm()) > 0, name
        errs[name] = float((b - a).norm() / a.norm())
    print(arch, "3x3 weight gradients, relative L2 on vs off:", {k: f"{v:.1e}" for k, v in errs.items()})
    for name, e in errs.items():
        assert e < 2e-2, f"grad {name}: relative L2 difference {e:.3e}"


def test_a_captured_step_at_batch_16_passes_the_replay_check_with_the_switch_on():
    """The model, data and settings of tests/test_graph_replay_gpu.py's misbehaves-under-replay test, default on_mismatch: with
    the 3x3 weight gradients off the stock split-K solver, the replayed step reproduces the eager one."""
    import mrla_amd
    from tests.test_graph_replay_gpu import _build, _data
    was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        with mrla_amd.conv3x3_wgrad():
            net = _build("resnet50_mrlal", 0.0)
            opt = torch.optim.SGD(net.parameters(), lr=0.02, momentum=0.9)
            x, y = _data(16)
            step = mrla_amd.graphed_step(net, opt, F.cross_entropy, (x, y), verify=3)
            print({k: step.report[k] for k in ("weights_rel_l2", "update_rel_l2", "worst_parameter")})
            assert step.report["ok"] and step.graph is not None
    finally:
        torch.backends.cudnn.benchmark = was
