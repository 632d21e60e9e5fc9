"""GPU: the opt-in route of the fp32 stem weight gradient in the Python layer (functional.stem_conv under
mrla_amd.stem_wgrad_f32()), for the recipe that trains in fp32 without autocast.

  * one fp32 Conv2d(3, 64, 7, 2, 3, bias=False) on a 2 x 3 x 9 x 6 channels_last input: with the switch on exactly one
    mrla_stem_conv_f32_wgrad launch per backward and none of mrla_stem_conv_wgrad (counted through functional._call); y
    bit-equal to conv(x); weight.grad fp32 [64, 3, 7, 7] in the weight's own strides -- channels_last and contiguous alike --
    inside (m + 9) * 2^-24 * A of the float64 CPU gradient (m = b * ho * wo output pixels, A the same gradient of |x|, |dy|:
    the bound of any fp32 summation order of m fused products).  Switch off, stem_wgrad() only, torch.no_grad() or a frozen
    weight: the module's own graph, zero launches.  Under bf16 autocast with both stem switches on only the 16-bit entry
    point runs;
  * resnet18_mrlal and resnet50_mrlal in fp32, batch 8 at 64 x 64, deterministic stock solvers, under
    reproducible_gradients(): one fp32 stem launch per backward; two steps from the same state are bit-equal in the loss and
    in conv1.weight.grad; the loss is bit-equal to that of the step with STEM_WGRAD_F32 alone switched off; with the stem's x
    and dy saved on both sides, BOTH conv1.weight.grads are inside the bound above of the float64 gradient of the saved
    tensors.  The on-against-off relative L2 is printed, not asserted."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_stem_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
OWN, OWN16 = "mrla_stem_conv_f32_wgrad", "mrla_stem_conv_wgrad"


class _Counter:
    """functional._call with the launches counted per entry point; the product code is not changed."""

    def __init__(self, monkeypatch):
        from mrla_amd import functional as Fm
        self.n, inner = {OWN: 0, OWN16: 0}, Fm._call

        def counted(label, *args, **kw):
            name = kw.get("entry") or label
            if name in self.n:
                self.n[name] += 1
            return inner(label, *args, **kw)
        monkeypatch.setattr(Fm, "_call", counted)


class _Deterministic:
    """Deterministic stock solvers inside the block: the stock side of a comparison has to agree with itself."""

    def __enter__(self):
        self.was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True

    def __exit__(self, *exc):
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = self.was


def _dw64(x, dy):
    w = torch.zeros((dy.shape[1], 3, 7, 7), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, w, stride=2, padding=3), w, dy)
    return g


def _inside_the_bound(gw, x, dy):
    """(all inside, max |gw - dw64| / A, the bound's factor) against the float64 CPU gradient of the device tensors x, dy."""
    x64, dy64 = x.detach().double().cpu(), dy.detach().double().cpu()
    want64, a = _dw64(x64, dy64), _dw64(x64.abs(), dy64.abs())
    m = dy64.shape[0] * dy64.shape[2] * dy64.shape[3]
    err = (gw.detach().double().cpu() - want64).abs()
    return bool((err <= (m + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max()), (m + 9) * 2.0 ** -24


def test_one_convolution(monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch)
    torch.manual_seed(3)
    stock = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=CL)
    ours = copy.deepcopy(stock)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((2, 3, 9, 6), device="cuda", generator=g).contiguous(memory_format=CL)
    dy = torch.randn((2, 64, 5, 3), device="cuda", generator=g).contiguous(memory_format=CL)
    assert Fm.stem_conv_f32_applies(ours, x) and not Fm.stem_conv_applies(ours, x)
    with _Deterministic():
        # ---- switch on ----
        ys = stock(x)
        with mrla_amd.stem_wgrad_f32():
            yo = Fm.stem_conv(x, ours)
        assert type(yo.grad_fn).__name__.startswith("_StemConvFn") and yo.dtype == torch.float32
        assert torch.equal(yo.view(torch.int32), ys.view(torch.int32))
        for i in range(1, 3):
            ours.weight.grad = None
            yo.backward(dy, retain_graph=True)
            assert count.n == {OWN: i, OWN16: 0}
            gw = ours.weight.grad
            assert gw.dtype == torch.float32 and gw.shape == (64, 3, 7, 7) and gw.stride() == ours.weight.stride()
            ok, ratio, bound = _inside_the_bound(gw, x, dy)
            print(f"one convolution: max |dw - dw64| / A = {ratio:.3e} (the bound {bound:.3e})")
            assert ok, ratio
        # a weight in other strides (channels_last above; contiguous here) gets its gradient in its own
        plain = copy.deepcopy(stock).to(memory_format=torch.contiguous_format)
        assert plain.weight.stride() != ours.weight.stride()
        with mrla_amd.stem_wgrad_f32():
            Fm.stem_conv(x, plain).backward(dy)
        assert count.n == {OWN: 3, OWN16: 0} and plain.weight.grad.stride() == plain.weight.stride()
        assert torch.equal(plain.weight.grad.contiguous().view(torch.int32), gw.contiguous().view(torch.int32))
        ok, ratio, _ = _inside_the_bound(plain.weight.grad, x, dy)
        assert ok, ratio
        count.n[OWN] = 0
        # ---- the 16-bit switch never routes fp32 ----
        with mrla_amd.stem_wgrad():
            y = Fm.stem_conv(x, ours)
            assert type(y.grad_fn) is type(ys.grad_fn) and torch.equal(y, ys)
            y.backward(dy)
        assert count.n == {OWN: 0, OWN16: 0}
        # ---- switch off: the module's own graph ----
        y = Fm.stem_conv(x, ours)
        assert type(y.grad_fn) is type(ys.grad_fn) and torch.equal(y, ys)
        y.backward(dy)
        assert count.n == {OWN: 0, OWN16: 0}
        # ---- no_grad and a frozen weight: the module itself ----
        with mrla_amd.stem_wgrad_f32():
            with torch.no_grad():
                assert not Fm.stem_conv_f32_applies(ours, x)
                y = Fm.stem_conv(x, ours)
                assert y.grad_fn is None and torch.equal(y, ys)
            frozen = copy.deepcopy(stock)
            frozen.weight.requires_grad_(False)
            xr = x.clone().requires_grad_(True)
            assert not Fm.stem_conv_f32_applies(frozen, xr)
            y = Fm.stem_conv(xr, frozen)
            assert type(y.grad_fn) is type(frozen(xr).grad_fn) and torch.equal(y, ys)
            y.backward(dy)
            assert frozen.weight.grad is None
        assert count.n == {OWN: 0, OWN16: 0}
        # ---- bf16 autocast with both stem switches on: only the 16-bit entry point ----
        ours.weight.grad = None
        with mrla_amd.stem_wgrad_f32(), mrla_amd.stem_wgrad(), torch.autocast("cuda", dtype=torch.bfloat16):
            assert Fm.stem_conv_applies(ours, x) and not Fm.stem_conv_f32_applies(ours, x)
            y = Fm.stem_conv(x, ours)
        assert y.dtype == torch.bfloat16
        y.backward(dy.bfloat16())
        assert count.n == {OWN: 0, OWN16: 1} and ours.weight.grad.dtype == torch.float32


def test_applies_refuses_the_excluded_configurations_on_the_device():
    from mrla_amd import functional as Fm
    for name, c, make in excluded_configurations():
        if name.startswith("fp32"):
            continue
        xe = make("cuda").float()
        assert not Fm.stem_conv_f32_applies(c.cuda().to(memory_format=CL), xe), name
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=CL)
    x = torch.randn(2, 3, 12, 12, device="cuda").contiguous(memory_format=CL)
    assert Fm.stem_conv_f32_applies(conv, x) and not Fm.stem_conv_applies(conv, x)
    assert not Fm.stem_conv_f32_applies(conv, x.bfloat16())                                       # bf16 input
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not Fm.stem_conv_f32_applies(conv, x)                                              # fp32 input under bf16 autocast
    assert not Fm.stem_conv_f32_applies(conv, x.contiguous())                                     # NCHW
    assert not Fm.stem_conv_f32_applies(copy.deepcopy(conv).double(), x)                          # the weight is not fp32
    assert not Fm.stem_conv_f32_applies(torch.nn.Conv2d(3, 96, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=CL), x)


def _model_step(arch, on, monkeypatch):
    """(loss, conv1.weight.grad, (x, dy) of the stem) of one fp32 step under reproducible_gradients(), STEM_WGRAD_F32 = on."""
    import contextlib
    import io
    import mrla_amd
    from mrla_amd import functional as Fm, models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(models, arch)(drop_path=0.0).cuda().to(memory_format=CL).train()
    with torch.no_grad():          # the blocks' last BatchNorm starts at weight 0: the gradient would reach the stem by the shortcuts alone
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    saved, inner = {}, Fm.stem_conv

    def recording(x, conv):
        y = inner(x, conv)
        assert conv is net.conv1 and x.is_contiguous(memory_format=CL) and x.data_ptr() % 16 == 0      # what the step hands the stem
        saved["x"] = x.detach()
        y.register_hook(lambda g: saved.__setitem__("dy", g.detach().clone()))
        return y
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, 3, 64, 64, device="cuda", generator=g)          # NCHW, as a data loader hands it over
    y = torch.randint(0, 1000, (8,), device="cuda", generator=g)
    with monkeypatch.context() as mp:
        mp.setattr(Fm, "stem_conv", recording)
        with mrla_amd.reproducible_gradients(), mrla_amd.stem_wgrad_f32(on):
            loss = F.cross_entropy(net(x), y)
            loss.backward()
    assert loss.dtype == torch.float32 and tuple(saved["x"].shape) == (8, 3, 64, 64) and saved["x"].dtype == torch.float32
    assert tuple(saved["dy"].shape) == (8, 64, 32, 32) and saved["dy"].dtype == torch.float32
    return loss.detach().clone(), net.conv1.weight.grad.detach().clone(), (saved["x"], saved["dy"])


@pytest.mark.parametrize("arch", ["resnet18_mrlal", "resnet50_mrlal"])
def test_an_fp32_model_step_is_reproducible_with_the_switch_on_and_close_to_the_step_with_it_off(arch, monkeypatch):
    count = _Counter(monkeypatch)
    with _Deterministic():
        loss1, gw1, s1 = _model_step(arch, True, monkeypatch)
        assert count.n == {OWN: 1, OWN16: 0}
        loss2, gw2, _ = _model_step(arch, True, monkeypatch)
        assert count.n == {OWN: 2, OWN16: 0}
        loss0, gw0, s0 = _model_step(arch, False, monkeypatch)
        assert count.n == {OWN: 2, OWN16: 0}
    # two steps from the same state with the switch on: bit-equal
    assert torch.equal(loss1.view(torch.int32), loss2.view(torch.int32)), (float(loss1), float(loss2))
    assert bool(torch.isfinite(gw1).all()) and float(gw1.norm()) > 0 and gw1.shape == (64, 3, 7, 7)
    assert torch.equal(gw1.view(torch.int32), gw2.view(torch.int32))
    # the forward is the stock operator's on both sides
    assert torch.equal(loss1.view(torch.int32), loss0.view(torch.int32)), (float(loss1), float(loss0))
    # on against off, through the float64 gradient of the stem's saved tensors: both sides inside the summation bound
    for side, gw, (x, dy) in (("on", gw1, s1), ("off", gw0, s0)):
        ok, ratio, bound = _inside_the_bound(gw, x, dy)
        print(f"{arch} conv1 ({side}): max |dw - dw64| / A = {ratio:.3e} (the bound {bound:.3e})")
        assert ok, (side, ratio)
    print(f"{arch}: loss {float(loss1)!r}; conv1.weight.grad, relative L2 on vs off: "
          f"{float((gw1.double() - gw0.double()).norm() / gw0.double().norm()):.3e}")
