"""GPU: the opt-in route of the own 3x3 forward in the Python layer (functional.conv3x3 / conv3x3_bn_act under
mrla_amd.conv3x3_fwd()).

  * conv3x3(x, conv) with the switch on against the stock module: the node is the new one, y and dx within 2 ulps of the
    16-bit type of the tensor's largest magnitude, y bit-equal to the direct C-ABI call, with conv3x3_wgrad() also on
    weight.grad bit-equal to the direct mrla_conv3x3_wgrad call, a second backward bit-equal to the first (the backwards run with
    torch.backends.cudnn.deterministic, for the stride-2 dx, which is the stock operator's);
  * launch counts, by wrapping functional._call: one mrla_conv3x3_fwd per forward, one more per backward at stride 1 when x
    wants its gradient, none at stride 2 in backward, none with the switch off or for an excluded configuration; under no_grad
    and for a frozen weight the forward still launches;
  * conv3x3_bn_act in train mode against conv -> BatchNorm2d -> relu in fp32 (the bounds of
    tests/test_conv1x1_gpu.py::test_conv_bn_act_composite_matches_stock_modules), without a mrla_bn_plane_moments launch; eval
    mode and defer=True against the switch-off result;
  * whole models: two steps from one state are bit-equal in the loss and every parameter gradient with all own switches on;
    the 3x3 weight gradients are no further from an fp32 step than the stock forward's; a captured step passes the replay check."""
import contextlib
import copy
import io

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_wgrad_cpu import excluded_configurations

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


class _Counter:
    """functional._call with the launches of every entry point counted; the product code is not changed."""

    def __init__(self, monkeypatch):
        from mrla_amd import functional as Fm
        self.counts, inner = {}, Fm._call

        def counted(label, *args, **kw):
            name = kw.get("entry") or label
            self.counts[name] = self.counts.get(name, 0) + 1
            return inner(label, *args, **kw)
        monkeypatch.setattr(Fm, "_call", counted)

    def n(self, name="mrla_conv3x3_fwd"):
        return self.counts.get(name, 0)


@contextlib.contextmanager
def _deterministic_stock():
    was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        yield
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = was


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 7, 7, 1), (2, 128, 128, 9, 6, 2)], ids=lambda s: "x".join(map(str, s)))
def test_the_route_against_the_stock_module(shape, dtype):
    import mrla_amd
    from mrla_amd import _lib as L, functional as Fm
    b, c, n, h, w, s = shape
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    torch.manual_seed(3)
    stock = torch.nn.Conv2d(c, n, 3, stride=s, padding=1, bias=False).cuda().to(memory_format=CL)
    ours = copy.deepcopy(stock)
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn((b, c, h, w), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    dy = torch.randn((b, n, ho, wo), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    xs, xo = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        ys = stock(xs)
        assert Fm.conv3x3_fwd_applies(ours, xo)
        with mrla_amd.conv3x3_fwd(), mrla_amd.conv3x3_wgrad():
            yo = Fm.conv3x3(xo, ours)
    assert type(yo.grad_fn).__name__.startswith("_Conv3x3FwdFn") and yo.dtype == dtype and yo.shape == ys.shape
    assert yo.is_contiguous(memory_format=CL)
    ys.backward(dy)
    with _deterministic_stock():          # (for the stride-2 dx, the stock operator's: its default solvers do not repeat themselves)
        yo.backward(dy, retain_graph=True)
    for name, got, want in (("y", yo, ys), ("dx", xo.grad, xs.grad)):
        err = float((got.detach().double() - want.detach().double()).abs().max())
        bound = 2 * ULP[dtype] * float(want.detach().double().abs().max())
        print(f"{shape} {dtype} {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err)
    # y bit-equal to the C ABI on the same x and the weight as autocast casts it
    w16 = ours.weight.detach().to(dtype).contiguous(memory_format=CL)
    direct = torch.empty((b, n, ho, wo), dtype=dtype, device="cuda", memory_format=CL)
    L.call("mrla_conv3x3_fwd", x0.data_ptr(), w16.data_ptr(), direct.data_ptr(), None, b, c, n, h, w, s, Fm._DT[dtype], Fm._stream())
    assert torch.equal(yo.detach().view(torch.int16), direct.view(torch.int16))
    # weight.grad bit-equal to the direct mrla_conv3x3_wgrad call on the same x, dy
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == (n, c, 3, 3) and gw.stride() == ours.weight.stride()
    rows = L.load().mrla_conv3x3_wgrad_rows(b, c, n, h, w, s, Fm._DT[dtype])
    part = torch.empty((rows, n, 9, c), dtype=torch.float32, device="cuda")
    dwd = torch.empty((n, c, 3, 3), dtype=torch.float32, device="cuda", memory_format=CL)
    L.call("mrla_conv3x3_wgrad", dy.data_ptr(), x0.data_ptr(), part.data_ptr(), dwd.data_ptr(), b, c, n, h, w, s, Fm._DT[dtype],
           L.F32, Fm._stream())
    assert torch.equal(gw.view(torch.int32), dwd.view(torch.int32))
    # ... and a second backward equals the first
    first_w, first_x = gw.clone(), xo.grad.clone()
    ours.weight.grad, xo.grad = None, None
    with _deterministic_stock():
        yo.backward(dy)
    assert torch.equal(ours.weight.grad.view(torch.int32), first_w.view(torch.int32))
    assert torch.equal(xo.grad.view(torch.int16), first_x.view(torch.int16))


def test_launch_counts(monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    count = _Counter(monkeypatch)
    conv1 = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).cuda().bfloat16().to(memory_format=CL)
    conv2 = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).cuda().bfloat16().to(memory_format=CL)
    x = torch.randn(2, 64, 6, 6, device="cuda").bfloat16().contiguous(memory_format=CL)
    with mrla_amd.conv3x3_fwd():
        y = Fm.conv3x3(x, conv1)                         # x wants no gradient: one launch forward, none backward
        assert count.n() == 1
        y.float().sum().backward()
        assert count.n() == 1 and conv1.weight.grad is not None
        xg = x.clone().requires_grad_(True)
        y = Fm.conv3x3(xg, conv1)                        # stride 1, x wants its gradient: one more per backward
        assert count.n() == 2
        y.float().sum().backward()
        assert count.n() == 3 and xg.grad is not None
        xg.grad = None
        y = Fm.conv3x3(xg, conv2)                        # stride 2: none in backward
        assert count.n() == 4
        y.float().sum().backward()
        assert count.n() == 4 and xg.grad is not None
        assert count.n("mrla_conv3x3_wgrad") == 0        # (that switch is off)
        with torch.no_grad():                            # inference still launches
            y = Fm.conv3x3(x, conv1)
        assert count.n() == 5 and not y.requires_grad
        want = conv1(x)
        assert float((y.double() - want.double()).abs().max()) <= 2 * ULP[torch.bfloat16] * float(want.double().abs().max())
    y = Fm.conv3x3(xg, conv1)                            # switch off: the module itself
    assert not type(y.grad_fn).__name__.startswith("_Conv3x3") and torch.equal(y, conv1(xg))
    y.float().sum().backward()
    assert count.n() == 5
    with mrla_amd.conv3x3_fwd():
        for name, c, make in excluded_configurations():
            xe = make("cuda")
            c = c.cuda().to(xe.dtype).to(memory_format=CL)
            before = count.n()
            ye = Fm.conv3x3(xe, c)
            if name == "frozen weight":                  # eligible for the forward
                assert Fm.conv3x3_fwd_applies(c, xe) and count.n() == before + 1
                want = c(xe)
                assert float((ye.double() - want.double()).abs().max()) <= 2 * ULP[torch.bfloat16] * float(want.double().abs().max())
                continue
            assert not Fm.conv3x3_fwd_applies(c, xe) and count.n() == before, name
            assert torch.equal(ye, c(xe)), name
            if ye.requires_grad:
                ye.float().sum().backward()
            assert count.n() == before, name


def _conv_bn(c, n, s):
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(c, n, 3, stride=s, padding=1, bias=False).cuda().to(memory_format=CL)
    bn = torch.nn.BatchNorm2d(n).cuda()
    with torch.no_grad():
        conv.weight.copy_(conv.weight.bfloat16().float())
        bn.weight.uniform_(0.8, 1.2)
        bn.bias.uniform_(-0.1, 0.1)
    return conv, bn


@pytest.mark.parametrize("sequences", [False, True], ids=["passes", "sequences"])
@pytest.mark.parametrize("shape", [(4, 64, 128, 14, 14, 1, True), (3, 128, 64, 9, 6, 2, False)], ids=lambda s: "x".join(map(str, s)))
def test_conv_bn_act_in_train_mode_matches_the_stock_modules(shape, sequences, monkeypatch):
    """Both BatchNorm routes: the single passes, whose launches functional._call sees, and the sequence entry point
    (mrla_bn_fwd, the default), which takes the records in the moments pass's place."""
    import mrla_amd
    from mrla_amd import functional as Fm
    b, c, n, h, w, s, relu = shape
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    monkeypatch.setattr(Fm, "SEQUENCES", sequences)
    count = _Counter(monkeypatch)
    conv, bn = _conv_bn(c, n, s)
    conv_r, bn_r = copy.deepcopy(conv), copy.deepcopy(bn)
    g = torch.Generator(device="cuda").manual_seed(17)
    xt = torch.randn((b, c, h, w), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL).requires_grad_(True)
    gup = torch.randn((b, n, ho, wo), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL)
    with mrla_amd.conv3x3_fwd(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = Fm.conv3x3_bn_act(xt, conv, bn, relu)
    out.backward(gup)
    assert count.n() == (2 if s == 1 else 1) and count.n("mrla_bn_plane_moments") == 0
    if not sequences:
        assert count.n("mrla_bn_stats_fwd_rows") == 1 and count.n("mrla_bn_stats_fwd") == 0
    # reference: fp32 modules on the same operands; the convolution output rounded to bf16 where the product stores it
    xr = xt.detach().float().requires_grad_(True)
    zr = bn_r(conv_r(xr).bfloat16().float())
    if relu:
        zr = torch.relu(zr)
    zr.backward(gup.float())
    a, r = out.detach().float(), zr.detach()
    bad = (a - r).abs() > 2.0 ** -7 * (r.abs() + 0.05 * r.abs().max())
    print(f"{shape}: outputs outside the bound {bad.float().mean().item():.2e}")
    assert bad.float().mean().item() < 1e-4
    assert torch.allclose(bn.running_mean, bn_r.running_mean, rtol=1e-4, atol=1e-6)
    assert torch.allclose(bn.running_var, bn_r.running_var, rtol=1e-4, atol=1e-6)
    for got, want in ((bn.weight.grad, bn_r.weight.grad), (bn.bias.grad, bn_r.bias.grad)):
        assert ((got.float() - want).norm() / want.norm()).item() < 2e-2


@pytest.mark.parametrize("mode", ["eval", "defer"])
def test_conv_bn_act_in_eval_mode_and_deferred_equals_the_switch_off_result(mode, monkeypatch):
    import mrla_amd
    from mrla_amd import functional as Fm
    monkeypatch.setattr(Fm, "SEQUENCES", False)          # (the single passes: functional._call sees their launches)
    count = _Counter(monkeypatch)
    conv, bn = _conv_bn(64, 64, 1)
    with torch.no_grad():
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    bn.train(mode == "defer")
    bn_off = copy.deepcopy(bn)
    g = torch.Generator(device="cuda").manual_seed(19)
    x = torch.randn((3, 64, 7, 7), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL)

    def run(on, bn_):
        with mrla_amd.conv3x3_fwd(on), torch.autocast("cuda", dtype=torch.bfloat16):
            y = Fm.conv3x3_bn_act(x, conv, bn_, relu=False, defer=mode == "defer")
        if mode == "defer":                              # the affine is the consumer's to apply
            sc, sh = y._mrla_affine
            return y.detach().float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        return y.detach().float()
    r = run(False, bn_off)
    assert count.n() == 0
    a = run(True, bn)
    assert count.n() == 1 and count.n("mrla_bn_plane_moments") == (1 if mode == "defer" else 0)     # (the switch-off run's)
    bad = (a - r).abs() > 2.0 ** -7 * (r.abs() + 0.05 * r.abs().max())
    assert bad.float().mean().item() < 1e-4


# ---- whole models ---------------------------------------------------------------------------------------------------

def _model_step(arch, fwd, repro, fp32=False, batch=16, side=96):
    """(loss, {parameter: gradient}, {3x3 conv weight: gradient}) of one step from a fixed state."""
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
    x = torch.randn(batch, 3, side, side, device="cuda", generator=g).contiguous(memory_format=CL)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    with mrla_amd.conv3x3_fwd(fwd), mrla_amd.reproducible_gradients(repro), torch.autocast("cuda", dtype=torch.bfloat16, enabled=not fp32):
        loss = F.cross_entropy(net(x), y)
        loss.backward()
    grads = {name: p.grad.clone() for name, p in net.named_parameters() if p.grad is not None}
    convs = [name + ".weight" for name, m in net.named_modules()
             if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1]     # (not the MRLA depthwise ones)
    return float(loss.detach()), grads, convs


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_two_model_steps_with_every_own_switch_on_are_bit_equal(arch, monkeypatch):
    count = _Counter(monkeypatch)
    with _deterministic_stock():
        loss0, g0, convs = _model_step(arch, True, True)
        n_fwd = count.n()
        loss1, g1, _ = _model_step(arch, True, True)
    # every 3x3 convolution of these models is eligible at this size: one forward launch each, one more for each stride-1 one
    # whose input wants its gradient (all of them: the stem in front is trained)
    from mrla_amd import models
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(models, arch)(drop_path=0.0)
    strides = [m.stride[0] for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1]
    assert len(strides) == len(convs) > 0 and n_fwd == len(strides) + strides.count(1), (n_fwd, strides)
    assert count.n() == 2 * n_fwd and count.n("mrla_conv3x3_wgrad") == 2 * len(convs)
    assert loss0 == loss1, (loss0, loss1)
    assert set(g0) == set(g1)
    differ = [k for k in g0 if not torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32))]
    assert not differ, f"{len(differ)} of {len(g0)} parameter gradients differ between two steps, first {differ[0]}"


@pytest.mark.parametrize("arch", ["resnet50_mrlal", "resnet18_mrlal"])
def test_the_own_forward_is_no_further_from_an_fp32_step_than_the_stock_one(arch):
    """The yardstick is neither side: the same step in fp32 without autocast, all switches off.  e = relative L2 of the
    concatenated 3x3 weight gradients against it; both bf16 sides make the same number of 16-bit roundings, so the expected
    ratio e_on / e_off is 1 and the margin of 1.5 is for the noise of one step.  Batch 16 at 96 x 96 (batch 8 at 64 x 64 is too
    ill-conditioned for any on/off comparison of a changed forward: profiles/conv3x3_wgrad.md section 6).

    Measured on MI355X (profiles/conv3x3_fwd.md section 4): e_off is NOT small here and does not fall with the image -- 0.46 for
    resnet50_mrlal and 0.18 for resnet18_mrlal at every size from 96 to 320 pixels: the distance between a bf16-autocast step
    and an fp32 step of these models, not noise that a larger image averages away -- so no size brings it under the 5 % that
    was hoped for, and 96 x 96 stays.  The ratio is what is asserted: e_on / e_off measured 0.99 .. 1.01 at all eight sizes.
    On against off measured 0.33 (resnet50_mrlal) and 0.105 (resnet18_mrlal): differences of an ulp in the forward, amplified by
    the train-mode BatchNorms over 144 samples per channel in the last stage, as section 6 of that file describes."""
    with _deterministic_stock():
        loss32, g32, convs = _model_step(arch, False, False, fp32=True)
        loss_off, g_off, _ = _model_step(arch, False, False)
        loss_on, g_on, _ = _model_step(arch, True, False)
    cat = lambda g: torch.cat([g[k].double().reshape(-1) for k in convs])  # noqa: E731
    ref = cat(g32)
    e_off = float((cat(g_off) - ref).norm() / ref.norm())
    e_on = float((cat(g_on) - ref).norm() / ref.norm())
    print(f"{arch}: e_off {e_off:.4e} e_on {e_on:.4e} losses fp32 {loss32!r} off {loss_off!r} on {loss_on!r}")
    assert e_on <= 1.5 * e_off, (e_on, e_off)
    # on against off directly.  The stock step at this size repeats itself bit for bit (also in find mode: measured), so there
    # is no run-to-run level to compare with; what bounds the distance is that on and off differ in a SUBSET of the roundings
    # that separate off from the fp32 step (the summation order inside the 3x3 forward and the stride-1 input gradient, fp32
    # accumulation and one rounding on both sides): on must be no further from off than the fp32 step is.
    off = cat(g_off)
    d = float((cat(g_on) - off).norm() / off.norm())
    print(f"{arch}: relative L2 of the 3x3 weight gradients, on against off: {d:.4e} (fp32 against off: {float((ref - off).norm() / off.norm()):.4e})")
    assert d <= float((ref - off).norm() / off.norm()), (d, e_off)


def test_a_captured_step_at_batch_16_passes_the_replay_check_with_all_three_switches_on():
    import mrla_amd
    from tests.test_graph_replay_gpu import _build, _data
    was = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        with mrla_amd.conv3x3_fwd(), mrla_amd.reproducible_gradients():
            net = _build("resnet50_mrlal", 0.0)
            opt = torch.optim.SGD(net.parameters(), lr=0.02, momentum=0.9)
            x, y = _data(16)
            step = mrla_amd.graphed_step(net, opt, F.cross_entropy, (x, y), verify=3)
            print({k: step.report[k] for k in ("weights_rel_l2", "update_rel_l2", "worst_parameter")})
            assert step.report["ok"] and step.graph is not None
    finally:
        torch.backends.cudnn.benchmark = was
