"""GPU: the opt-in route of the fp32 3x3 weight gradient in the Python layer (functional.conv3x3 under
mrla_amd.conv3x3_wgrad_f32()), for the recipe that trains in fp32 without autocast.

  * one fp32 Conv2d(64, 128, 3, stride s) on a 2 x 64 x 9 x 6 input: with the switch on exactly one mrla_conv3x3_f32_wgrad
    launch per backward and none of mrla_conv3x3_wgrad (counted through functional._call); y bit-equal to conv(x); under
    torch.backends.cudnn.deterministic x.grad bit-equal to the module's; weight.grad fp32, in the weight's strides, inside
    (m + 9) * 2^-24 * A of the float64 CPU gradient (m = b * ho * wo output pixels, A the same gradient of |x|, |dy|: the
    bound of any fp32 summation order of m fused products).  Switch off, torch.no_grad() or a frozen weight: the module itself;
  * resnet18_mrlal and resnet50_mrlal in fp32, batch 16 at 96 x 96: two steps from the same state with the switch on are
    bit-equal in the loss and in every 3x3 weight gradient, one launch per 3x3 group-1 convolution;
  * the same step with the switch off is the yardstick for closeness: for one stage-4 convolution (512 -> 512 on a 3 x 3
    map), x and dy are saved on both sides and BOTH weight gradients must be inside the bound above of the float64 CPU
    gradient of the saved tensors -- not inside a number picked in advance of each other.  The on-against-off relative L2
    over all 3x3 weight gradients is printed."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
OWN, OWN16 = "mrla_conv3x3_f32_wgrad", "mrla_conv3x3_wgrad"


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


def _dw64(x, dy, s):
    n, c = dy.shape[1], x.shape[1]
    w = torch.zeros((n, c, 3, 3), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, w, stride=s, padding=1), w, dy)
    return g


def _inside_the_bound(gw, x, dy, s):
    """(all inside, max |gw - dw64| / A) against the float64 CPU gradient of the device tensors x, dy."""
    x64, dy64 = x.detach().double().cpu(), dy.detach().double().cpu()
    want64, a = _dw64(x64, dy64, s), _dw64(x64.abs(), dy64.abs(), s)
    m = dy64.shape[0] * dy64.shape[2] * dy64.shape[3]
    err = (gw.detach().double().cpu() - want64).abs()
    return bool((err <= (m + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max())


@pytest.mark.parametrize("s", [1, 2])
def test_one_convolution(s, monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch)
    torch.manual_seed(3)
    stock = torch.nn.Conv2d(64, 128, 3, stride=s, padding=1, bias=False).cuda().to(memory_format=CL)
    ours = copy.deepcopy(stock)
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn((2, 64, 9, 6), device="cuda", generator=g).contiguous(memory_format=CL)
    ho, wo = (9 - 1) // s + 1, (6 - 1) // s + 1
    dy = torch.randn((2, 128, ho, wo), device="cuda", generator=g).contiguous(memory_format=CL)
    xs, xo = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    assert Fm.conv3x3_f32_applies(ours, xo) and not Fm.conv3x3_applies(ours, xo)
    with _Deterministic():
        # ---- switch on ----
        ys = stock(xs)
        with mrla_amd.conv3x3_wgrad_f32():
            yo = Fm.conv3x3(xo, ours)
        assert type(yo.grad_fn).__name__.startswith("_Conv3x3Fn") and yo.dtype == torch.float32
        assert torch.equal(yo.view(torch.int32), ys.view(torch.int32))
        ys.backward(dy)
        for i in range(1, 3):
            ours.weight.grad = xo.grad = None
            yo.backward(dy, retain_graph=True)
            assert count.n == {OWN: i, OWN16: 0}
            assert torch.equal(xo.grad.view(torch.int32), xs.grad.view(torch.int32))
            gw = ours.weight.grad
            assert gw.dtype == torch.float32 and gw.shape == (128, 64, 3, 3) and gw.stride() == ours.weight.stride()
            ok, ratio = _inside_the_bound(gw, x0, dy, s)
            print(f"stride {s}: max |dw - dw64| / A = {ratio:.3e} (the bound {(2 * ho * wo + 9) * 2.0 ** -24:.3e})")
            assert ok, ratio
        # a weight in other strides (channels_last here; contiguous below) gets its gradient in its own
        plain = copy.deepcopy(stock).to(memory_format=torch.contiguous_format)
        assert plain.weight.stride() != ours.weight.stride()
        with mrla_amd.conv3x3_wgrad_f32():
            Fm.conv3x3(x0, plain).backward(dy)
        assert count.n == {OWN: 3, OWN16: 0} and plain.weight.grad.stride() == plain.weight.stride()
        assert torch.equal(plain.weight.grad.contiguous().view(torch.int32), gw.contiguous().view(torch.int32))
        # ---- the 16-bit switches never route fp32 ----
        count.n[OWN] = 0
        with mrla_amd.conv3x3_wgrad(), mrla_amd.conv3x3_wgrad_auto():
            y = Fm.conv3x3(xo, ours)
            assert not type(y.grad_fn).__name__.startswith("_Conv3x3Fn")
        # ---- switch off: the module's own graph ----
        y = Fm.conv3x3(xo, ours)
        assert type(y.grad_fn) is type(stock(xs).grad_fn) and torch.equal(y, ys)
        y.backward(dy)
        assert count.n == {OWN: 0, OWN16: 0}
        # ---- no_grad and a frozen weight: the module itself ----
        with mrla_amd.conv3x3_wgrad_f32():
            with torch.no_grad():
                assert not Fm.conv3x3_f32_applies(ours, xo)
                y = Fm.conv3x3(xo, ours)
                assert y.grad_fn is None and torch.equal(y, ys)
            frozen = copy.deepcopy(stock)
            frozen.weight.requires_grad_(False)
            assert not Fm.conv3x3_f32_applies(frozen, xo)
            y = Fm.conv3x3(xo, frozen)
            assert type(y.grad_fn) is type(frozen(xo).grad_fn) and torch.equal(y, ys)
            y.backward(dy)
            assert frozen.weight.grad is None
        assert count.n == {OWN: 0, OWN16: 0}


def test_applies_refuses_the_excluded_configurations_on_the_device():
    from mrla_amd import functional as Fm
    for name, c, make in excluded_configurations():
        if name == "fp32":
            continue
        xe = make("cuda").float()
        assert not Fm.conv3x3_f32_applies(c.cuda().to(memory_format=CL), xe), name
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).cuda().to(memory_format=CL)
    x = torch.randn(2, 64, 6, 6, device="cuda").contiguous(memory_format=CL)
    assert Fm.conv3x3_f32_applies(conv, x)
    assert not Fm.conv3x3_f32_applies(conv, x.bfloat16())                                        # bf16 input
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not Fm.conv3x3_f32_applies(conv, x)                                               # fp32 input under bf16 autocast
    assert not Fm.conv3x3_f32_applies(conv, x.contiguous())                                      # NCHW
    assert not Fm.conv3x3_f32_applies(copy.deepcopy(conv).double(), x)                           # the weight is not fp32


def _model_step(arch, on, monkeypatch):
    """(loss, {name: 3x3 weight gradient}, (x, dy, gw) of the last 512 -> 512 stride-1 convolution) of one fp32 step."""
    import contextlib
    import io
    import mrla_amd
    from mrla_amd import functional as Fm, models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(models, arch)(drop_path=0.0).cuda().to(memory_format=CL).train()
    with torch.no_grad():          # the blocks' last BatchNorm starts at weight 0: every 3x3 weight gradient would be exactly 0
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    convs = {name: m for name, m in net.named_modules()
             if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1}     # (not the MRLA depthwise ones)
    watched = [m for m in convs.values() if m.in_channels == m.out_channels == 512 and m.stride == (1, 1)][-1]
    saved, inner = {}, Fm.conv3x3

    def recording(x, conv):
        y = inner(x, conv)
        if conv is watched:
            saved["x"] = x.detach()
            y.register_hook(lambda g: saved.__setitem__("dy", g.detach().clone()))
        return y
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(16, 3, 96, 96, device="cuda", generator=g).contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (16,), device="cuda", generator=g)
    with monkeypatch.context() as mp:
        mp.setattr(Fm, "conv3x3", recording)
        with mrla_amd.conv3x3_wgrad_f32(on):
            loss = F.cross_entropy(net(x), y)
            loss.backward()
    assert loss.dtype == torch.float32 and tuple(saved["x"].shape) == (16, 512, 3, 3) and saved["x"].dtype == torch.float32
    grads = {name + ".weight": m.weight.grad.detach().clone() for name, m in convs.items()}
    return loss.detach().clone(), grads, (saved["x"], saved["dy"], watched.weight.grad.detach().clone())


@pytest.mark.parametrize("arch", ["resnet18_mrlal", "resnet50_mrlal"])
def test_an_fp32_model_step_is_reproducible_with_the_switch_on_and_close_to_the_step_with_it_off(arch, monkeypatch):
    count = _Counter(monkeypatch)
    with _Deterministic():
        loss1, g1, w1 = _model_step(arch, True, monkeypatch)
        per_step = dict(count.n)
        loss2, g2, _ = _model_step(arch, True, monkeypatch)
        assert count.n == {OWN: 2 * per_step[OWN], OWN16: 0}
        loss0, g0, w0 = _model_step(arch, False, monkeypatch)
        assert count.n == {OWN: 2 * per_step[OWN], OWN16: 0}
    assert per_step == {OWN: len(g1), OWN16: 0} and len(g1) > 0      # every 3x3 group-1 convolution of these models is eligible
    # two steps from the same state with the switch on: bit-equal
    assert torch.equal(loss1.view(torch.int32), loss2.view(torch.int32)), (float(loss1), float(loss2))
    for name, a in g1.items():
        assert bool(torch.isfinite(a).all()) and float(a.norm()) > 0, name
        assert torch.equal(a.view(torch.int32), g2[name].view(torch.int32)), name
    # on against off, through the float64 gradient of one stage-4 convolution: both sides inside the summation bound
    for side, (x, dy, gw) in (("on", w1), ("off", w0)):
        ok, ratio = _inside_the_bound(gw, x, dy, 1)
        print(f"{arch} stage-4 3x3 ({side}): max |dw - dw64| / A = {ratio:.3e} (the bound {(16 * 9 + 9) * 2.0 ** -24:.3e})")
        assert ok, (side, ratio)
    on, off = (torch.cat([g[k].double().flatten() for k in sorted(g)]) for g in (g1, g0))
    print(f"{arch}: losses off {float(loss0)!r} on {float(loss1)!r}; 3x3 weight gradients, relative L2 on vs off: "
          f"{float((on - off).norm() / off.norm()):.3e}")
