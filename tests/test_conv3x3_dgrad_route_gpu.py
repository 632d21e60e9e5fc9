"""GPU: the opt-in route of the own stride-2 3x3 input gradient in the Python layer (functional.conv3x3 / conv3x3_bn_act under
mrla_amd.conv3x3_dgrad()).

  * launch counts, by wrapping functional._call: one mrla_conv3x3_dgrad_s2 per stride-2 backward when x wants its gradient;
    none at stride 1, when x wants no gradient, for an excluded configuration or with the switch off;
  * conv3x3(x, conv) against the stock module: under the new switch alone y is bit-equal (it IS the stock forward) and dx
    within 2 ulps of the 16-bit type of the tensor's largest magnitude; under all four switches dx and weight.grad within the
    same bound; dx bit-equal to the direct C-ABI call; a second backward bit-equal to the first WITHOUT
    torch.backends.cudnn.deterministic (no product of the call site is the stock library's any more);
  * whole models with all four switches on: one launch per stride-2 3x3 convolution per step, two steps from one state
    bit-equal in the loss and every parameter gradient, the 3x3 weight gradients no further from the same step with the new
    switch off than an fp32 step is; a captured step passes the replay check."""
import contextlib
import copy
import io

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_fwd_route_gpu import ULP, _Counter, _deterministic_stock
from tests.test_conv3x3_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ENTRY = "mrla_conv3x3_dgrad_s2"


@contextlib.contextmanager
def _all_four(dgrad=True):
    import mrla_amd
    with mrla_amd.conv3x3_fwd(), mrla_amd.reproducible_gradients(), mrla_amd.conv3x3_dgrad(dgrad):
        yield


@pytest.fixture
def _stock_repeats_itself():
    """The stock library's deterministic solvers for a test that compares two stock forwards bit for bit."""
    with _deterministic_stock():
        yield


def test_launch_counts(monkeypatch, _stock_repeats_itself):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch)
    conv1 = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).cuda().bfloat16().to(memory_format=CL)
    conv2 = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).cuda().bfloat16().to(memory_format=CL)
    x = torch.randn(2, 64, 6, 6, device="cuda").bfloat16().contiguous(memory_format=CL)
    xg = x.clone().requires_grad_(True)
    with mrla_amd.conv3x3_dgrad():
        assert Fm.conv3x3_dgrad_applies(conv2, xg) and not Fm.conv3x3_dgrad_applies(conv2, x)
        assert not Fm.conv3x3_dgrad_applies(conv1, xg)
        with torch.no_grad():
            assert not Fm.conv3x3_dgrad_applies(conv2, xg)
        y = Fm.conv3x3(xg, conv2)                        # stride 2, x wants its gradient: the stock forward, one launch backward
        assert type(y.grad_fn).__name__.startswith("_Conv3x3Fn") and torch.equal(y, conv2(xg))
        assert count.n(ENTRY) == 0
        y.float().sum().backward(retain_graph=True)
        assert count.n(ENTRY) == 1 and xg.grad is not None and conv2.weight.grad is not None
        y.float().sum().backward()                       # ... per backward
        assert count.n(ENTRY) == 2
        assert count.n("mrla_conv3x3_wgrad") == 0 and count.n("mrla_conv3x3_fwd") == 0      # (those switches are off)
        y = Fm.conv3x3(x, conv2)                         # x wants no gradient: the module itself
        assert not type(y.grad_fn).__name__.startswith("_Conv3x3") and torch.equal(y, conv2(x))
        y.float().sum().backward()
        assert count.n(ENTRY) == 2
        y = Fm.conv3x3(xg, conv1)                        # stride 1: the module itself
        assert not type(y.grad_fn).__name__.startswith("_Conv3x3") and torch.equal(y, conv1(xg))
        y.float().sum().backward()
        assert count.n(ENTRY) == 2
        with mrla_amd.conv3x3_fwd():                     # the own forward's node: the same decision, the same launch
            y = Fm.conv3x3(xg, conv2)
            assert type(y.grad_fn).__name__.startswith("_Conv3x3FwdFn")
            y.float().sum().backward()
            assert count.n(ENTRY) == 3
            y = Fm.conv3x3(x, conv2)                     # ... and none when x wants no gradient
            y.float().sum().backward()
            y = Fm.conv3x3(xg, conv1)                    # ... or at stride 1
            y.float().sum().backward()
            assert count.n(ENTRY) == 3
        for name, c, make in excluded_configurations():
            xe = make("cuda").requires_grad_(True)
            c = c.cuda().to(xe.dtype).to(memory_format=CL)
            assert not Fm.conv3x3_dgrad_applies(c, xe), name
            ye = Fm.conv3x3(xe, c)
            assert torch.equal(ye, c(xe)) and not type(ye.grad_fn).__name__.startswith("_Conv3x3"), name
            ye.float().sum().backward()
            assert count.n(ENTRY) == 3, name
    y = Fm.conv3x3(xg, conv2)                            # switch off: the module itself
    assert not type(y.grad_fn).__name__.startswith("_Conv3x3") and torch.equal(y, conv2(xg))
    y.float().sum().backward()
    with mrla_amd.conv3x3_fwd(), mrla_amd.conv3x3_wgrad():
        Fm.conv3x3(xg, conv2).float().sum().backward()
    assert count.n(ENTRY) == 3


@pytest.mark.parametrize("shape,dtype", [((2, 64, 64, 7, 7), torch.bfloat16), ((2, 64, 64, 9, 6), torch.bfloat16),
                                         ((2, 128, 128, 14, 14), torch.float16)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1])
def test_the_route_against_the_stock_module(shape, dtype):
    import mrla_amd
    from mrla_amd import _lib as L, functional as Fm
    b, c, n, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    torch.manual_seed(3)
    stock = torch.nn.Conv2d(c, n, 3, stride=2, padding=1, bias=False).cuda().to(memory_format=CL)
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn((b, c, h, w), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    dy = torch.randn((b, n, ho, wo), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    xs = x0.clone().requires_grad_(True)
    # (the stock library's deterministic solvers for everything that is compared bit for bit with it or is its own on both
    # sides: in find mode two calls of the stock forward on the same operands need not return the same bits)
    with _deterministic_stock():
        with torch.autocast("cuda", dtype=dtype):
            ys = stock(xs)
        ys.backward(dy)

    def bound_check(name, got, want):
        err = float((got.detach().double() - want.detach().double()).abs().max())
        bound = 2 * ULP[dtype] * float(want.detach().double().abs().max())
        print(f"{shape} {dtype} {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err)

    # the direct C-ABI call on the same dy and the weight as autocast casts it
    w16 = stock.weight.detach().to(dtype).contiguous(memory_format=CL)
    direct = torch.empty_like(x0)
    L.call(ENTRY, dy.data_ptr(), w16.data_ptr(), direct.data_ptr(), b, c, n, h, w, Fm._DT[dtype], Fm._stream())

    # ---- the new switch alone: the stock forward, the stock weight gradient, the own dx ----
    ours, xo = copy.deepcopy(stock), x0.clone().requires_grad_(True)
    ours.weight.grad = None
    with _deterministic_stock(), torch.autocast("cuda", dtype=dtype), mrla_amd.conv3x3_dgrad():
        assert Fm.conv3x3_dgrad_applies(ours, xo)
        yo = Fm.conv3x3(xo, ours)
    assert type(yo.grad_fn).__name__.startswith("_Conv3x3Fn") and yo.dtype == dtype
    assert torch.equal(yo.detach().view(torch.int16), ys.detach().view(torch.int16))
    with _deterministic_stock():          # (for the weight gradient, the stock operator's under this switch alone)
        yo.backward(dy)
    bound_check("dx, the switch alone", xo.grad, xs.grad)
    assert torch.equal(xo.grad.view(torch.int16), direct.view(torch.int16))
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == (n, c, 3, 3) and gw.stride() == ours.weight.stride()
    bound_check("dw, the switch alone", gw, stock.weight.grad)

    # ---- all four switches: no product is the stock library's, so the backward repeats itself as it is ----
    ours, xo = copy.deepcopy(stock), x0.clone().requires_grad_(True)
    ours.weight.grad = None
    with torch.autocast("cuda", dtype=dtype), _all_four():
        yo = Fm.conv3x3(xo, ours)
    assert type(yo.grad_fn).__name__.startswith("_Conv3x3FwdFn")
    yo.backward(dy, retain_graph=True)
    bound_check("y, all four", yo, ys)
    bound_check("dx, all four", xo.grad, xs.grad)
    bound_check("dw, all four", ours.weight.grad, stock.weight.grad)
    assert torch.equal(xo.grad.view(torch.int16), direct.view(torch.int16))
    first_w, first_x = ours.weight.grad.clone(), xo.grad.clone()
    ours.weight.grad, xo.grad = None, None
    yo.backward(dy)
    assert torch.equal(ours.weight.grad.view(torch.int32), first_w.view(torch.int32))
    assert torch.equal(xo.grad.view(torch.int16), first_x.view(torch.int16))


# ---- whole models ---------------------------------------------------------------------------------------------------

def _model_step(arch, dgrad, fp32=False, batch=16, side=96):
    """(loss, {parameter: gradient}, [3x3 conv weight names]) of one step from a fixed state: fp32 with every switch off, else
    bf16 autocast with CONV3X3_FWD, CONV3X3_WGRAD and STEM_WGRAD on and CONV3X3_DGRAD = `dgrad`."""
    from mrla_amd import models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(models, arch)(drop_path=0.0).cuda().to(memory_format=CL).train()
    with torch.no_grad():          # the blocks' last BatchNorm starts at weight 0: every 3x3 weight gradient would be exactly 0
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(batch, 3, side, side, device="cuda", generator=g).contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    switches = contextlib.nullcontext() if fp32 else _all_four(dgrad)
    with switches, torch.autocast("cuda", dtype=torch.bfloat16, enabled=not fp32):
        loss = F.cross_entropy(net(x), y)
        loss.backward()
    grads = {name: p.grad.clone() for name, p in net.named_parameters() if p.grad is not None}
    convs = [(name + ".weight", m.stride[0]) for name, m in net.named_modules()
             if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1]     # (not the MRLA depthwise ones)
    return float(loss.detach()), grads, convs


@pytest.fixture(scope="module")
def _steps():
    """The steps of a model that more than one test reads, run once: {(arch, kind): (loss, grads, convs)}."""
    cache = {}

    def get(arch, kind):
        if (arch, kind) not in cache:
            with _deterministic_stock():      # (for the stem forward and what else stays the stock library's)
                cache[arch, kind] = _model_step(arch, kind == "on", fp32=kind == "fp32")
        return cache[arch, kind]
    return get


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_two_model_steps_with_all_four_switches_on_are_bit_equal(arch, monkeypatch, _steps):
    count = _Counter(monkeypatch)
    with _deterministic_stock():
        loss1, g1, convs = _model_step(arch, True)
    strided = [name for name, s in convs if s == 2]
    assert len(strided) == 3 and count.n(ENTRY) == len(strided), (count.n(ENTRY), strided)
    assert count.n("mrla_conv3x3_wgrad") == len(convs)
    loss0, g0, _ = _steps(arch, "on")
    assert loss0 == loss1, (loss0, loss1)
    assert set(g0) == set(g1)
    differ = [k for k in g0 if not torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32))]
    assert not differ, f"{len(differ)} of {len(g0)} parameter gradients differ between two steps, first {differ[0]}"


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_the_own_input_gradient_is_no_further_from_the_switch_off_step_than_an_fp32_step(arch, _steps):
    """On (all four switches) against off (the other three) differ in the summation order inside three input gradients, fp32
    accumulation and one rounding on both sides: a SUBSET of the roundings that separate the bf16 step from the same step in
    fp32 without autocast.  So the relative L2 of the concatenated 3x3 weight gradients, on against off, must be no larger
    than fp32 against off; neither side of that yardstick is the code under test."""
    _, g32, convs = _steps(arch, "fp32")
    _, g_off, _ = _steps(arch, "off")
    _, g_on, _ = _steps(arch, "on")
    cat = lambda g: torch.cat([g[k].double().reshape(-1) for k, _ in convs])  # noqa: E731
    off = cat(g_off)
    d = float((cat(g_on) - off).norm() / off.norm())
    d32 = float((cat(g32) - off).norm() / off.norm())
    print(f"{arch}: relative L2 of the 3x3 weight gradients, on against off: {d:.4e} (fp32 against off: {d32:.4e})")
    assert d <= d32, (d, d32)


def test_a_captured_step_at_batch_16_passes_the_replay_check_with_all_four_switches_on():
    import mrla_amd
    from tests.test_graph_replay_gpu import _build, _data
    was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        with _all_four():
            net = _build("resnet50_mrlal", 0.0)
            opt = torch.optim.SGD(net.parameters(), lr=0.02, momentum=0.9)
            x, y = _data(16)
            step = mrla_amd.graphed_step(net, opt, F.cross_entropy, (x, y), verify=3)
            print({k: step.report[k] for k in ("weights_rel_l2", "update_rel_l2", "worst_parameter")})
            assert step.report["ok"] and step.graph is not None
    finally:
        torch.backends.cudnn.benchmark = was
