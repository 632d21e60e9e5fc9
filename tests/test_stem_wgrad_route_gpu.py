"""GPU: the opt-in route of the stem's weight gradient in the Python layer (functional.stem_conv under mrla_amd.stem_wgrad()).

  * stem_conv(x, conv) with the switch on against the stock module under autocast: out (and dX, asked for here although the
    product path never does) come from the same aten calls (within 2 ulps of the 16-bit type of the tensor's largest
    magnitude), conv.weight.grad is fp32 [64, 3, 7, 7] with the weight's strides, inside the fp32 summation bound of
    tests/test_stem_wgrad_gpu.py against float64, bit-equal to the direct C-ABI call on the same x, dy, and bit-equal on a
    second backward;
  * launch counts, by wrapping functional._call: once per backward where it applies, never with the switch off, under no_grad
    or for an excluded configuration, whose result is conv(x)'s;
  * whole models, one step with the switch off and on: the same loss within 2 bf16 ulps, conv1.weight.grad within the 2 %
    relative L2 that tests/test_block_bf16_gpu.py asks of parameter gradients, all gradients finite, exactly one launch;
  * a captured training step at batch 16 passes graphed_step's self-check under mrla_amd.reproducible_gradients()."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_route_gpu import _Counter
from tests.test_stem_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
ENTRY = "mrla_stem_conv_wgrad"


def _pair():
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    return conv, copy.deepcopy(conv)


def _dw64(x, dy):
    w = torch.zeros((dy.shape[1], 3, 7, 7), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, w, stride=2, padding=3), w, dy)
    return g


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 3, 9, 6)], ids=lambda s: "x".join(map(str, s)))
def test_the_route_against_the_stock_module(shape, dtype):
    import mrla_amd
    from mrla_amd import _lib as L, functional as Fm
    b, c, h, w = shape
    n, ho, wo = 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    stock, ours = _pair()
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    dy = torch.randn((b, n, ho, wo), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    xs, xo = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        ys = stock(xs)
        assert Fm.stem_conv_applies(ours, xo)
        with mrla_amd.stem_wgrad():
            yo = Fm.stem_conv(xo, ours)
    assert type(yo.grad_fn).__name__.startswith("_StemConvFn") and yo.dtype == dtype and yo.shape == ys.shape
    ys.backward(dy)
    yo.backward(dy, retain_graph=True)
    for name, got, want in (("out", yo, ys), ("dx", xo.grad, xs.grad)):
        err = float((got.double() - want.double()).abs().max())
        assert err <= 2 * ULP[dtype] * float(want.double().abs().max()), (name, err)
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == (n, 3, 7, 7) and gw.stride() == ours.weight.stride()
    # the fp32 summation bound against float64 (tests/test_stem_wgrad_gpu.py, item 2)
    x64, dy64 = x0.double().cpu(), dy.double().cpu()
    want64, a = _dw64(x64, dy64), _dw64(x64.abs(), dy64.abs())
    err = (gw.double().cpu() - want64).abs()
    assert bool((err <= (b * ho * wo + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max())
    # ... bit-equal to the C ABI on the same x, dy
    rows = L.load().mrla_stem_conv_wgrad_rows(b, n, h, w, Fm._DT[dtype])
    part = torch.empty((rows, n, 147), dtype=torch.float32, device="cuda")
    direct = torch.empty((n, 3, 7, 7), dtype=torch.float32, device="cuda", memory_format=CL)
    L.call(ENTRY, dy.data_ptr(), x0.data_ptr(), part.data_ptr(), direct.data_ptr(), b, n, h, w, Fm._DT[dtype], L.F32, Fm._stream())
    assert torch.equal(gw.contiguous().view(torch.int32), direct.contiguous().view(torch.int32))
    # ... and on a second backward
    first = gw.clone()
    ours.weight.grad = None
    yo.backward(dy)
    assert torch.equal(ours.weight.grad.view(torch.int32), first.view(torch.int32))


def test_one_launch_per_backward_where_it_applies_and_none_elsewhere(monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch, ENTRY)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().bfloat16()
    x = torch.randn(2, 3, 12, 12, device="cuda").bfloat16().contiguous(memory_format=CL)
    with mrla_amd.stem_wgrad():
        for i in range(1, 4):                            # eligible, switch on: once per backward
            Fm.stem_conv(x, conv).float().sum().backward()
            assert count.n == i
    count.n = 0
    y = Fm.stem_conv(x, conv)                            # switch off: the module itself
    assert torch.equal(y, conv(x)) and type(y.grad_fn).__name__ == type(conv(x).grad_fn).__name__
    y.float().sum().backward()
    assert count.n == 0
    with mrla_amd.stem_wgrad():
        with torch.no_grad():
            assert torch.equal(Fm.stem_conv(x, conv), conv(x))
        for name, c, make in excluded_configurations():
            xe = make("cuda")
            c = c.cuda().to(xe.dtype)
            assert not Fm.stem_conv_applies(c, xe), name
            ye = Fm.stem_conv(xe, c)
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
    with torch.no_grad():          # the blocks' last BatchNorm starts at weight 0: the gradient would reach the stem by the shortcuts alone
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, 3, 64, 64, device="cuda", generator=g).contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (8,), device="cuda", generator=g)
    with mrla_amd.stem_wgrad(on), torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(net(x), y)
        loss.backward()
    grads = {name: p.grad.double().cpu() for name, p in net.named_parameters() if p.grad is not None}
    return float(loss), grads


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_a_model_step_with_the_switch_on_matches_the_step_with_it_off(arch, monkeypatch):
    """One step each with the switch off and on, same seed, both under torch.backends.cudnn.deterministic (the stock 3x3 forward
    is not bit-stable at this size otherwise: profiles/conv3x3_wgrad.md section 6): the same loss within 2 bf16 ulps,
    conv1.weight.grad within the 2 % relative L2 of tests/test_block_bf16_gpu.py, all gradients finite, exactly one launch."""
    count = _Counter(monkeypatch, ENTRY)
    was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        loss0, g0 = _model_step(arch, False)
        assert count.n == 0
        loss1, g1 = _model_step(arch, True)
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = was
    print(arch, f"losses off {loss0!r} on {loss1!r}")
    assert count.n == 1
    ulp = 2.0 ** (torch.tensor(abs(loss0)).log2().floor().item() - 7)
    assert abs(loss1 - loss0) <= 2 * ulp, (loss0, loss1)
    assert g0.keys() == g1.keys() and "conv1.weight" in g1
    for name, b in g1.items():
        assert bool(torch.isfinite(b).all()), name
    a, b = g0["conv1.weight"], g1["conv1.weight"]
    assert b.shape == (64, 3, 7, 7) and float(a.norm()) > 0 and float(b.norm()) > 0
    e = float((b - a).norm() / a.norm())
    print(arch, f"conv1.weight.grad, relative L2 on vs off: {e:.3e}")
    assert e < 2e-2, f"grad conv1.weight: relative L2 difference {e:.3e}"


def test_a_captured_step_at_batch_16_passes_the_replay_check_under_reproducible_gradients():
    """The set-up of tests/test_conv3x3_route_gpu.py's captured-step test, with both switches on."""
    import mrla_amd
    from mrla_amd import functional as Fm
    from tests.test_graph_replay_gpu import _build, _data
    was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        with mrla_amd.reproducible_gradients():
            assert Fm.STEM_WGRAD and Fm.CONV3X3_WGRAD
            net = _build("resnet50_mrlal", 0.0)
            opt = torch.optim.SGD(net.parameters(), lr=0.02, momentum=0.9)
            x, y = _data(16)
            step = mrla_amd.graphed_step(net, opt, F.cross_entropy, (x, y), verify=3)
            print({k: step.report[k] for k in ("weights_rel_l2", "update_rel_l2", "worst_parameter")})
            assert step.report["ok"] and step.graph is not None
    finally:
        torch.backends.cudnn.benchmark = was
