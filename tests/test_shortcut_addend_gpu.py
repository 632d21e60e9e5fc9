"""The shortcut gradient inside conv1's input-gradient GEMM, in every kernel form (mrla_conv1x1_fwd_addend), and the wiring
that brings it there without a full-size tensor for the strided first blocks (resnet_mrla_light.py:91-114, 196-199).

Kernel level, through the C ABI: every form and mode against the path it replaces ON THE SAME INPUTS, bit for bit
(torch.equal, which treats -0 and +0 as equal: the only possible difference, at pixels that receive no addend):
  * wide form (n % 256 == 0, k <= 256), compact addend  ==  mrla_conv1x1_fwd_add with the addend scattered into zeros
    (same fp32 sum, same single rounding), and within 1 bf16 ulp of a float64 product + addend;
  * narrow form and both K-streaming tile forms, full-size and compact addend  ==  mrla_conv1x1_fwd followed by torch's
    bf16 add of the (scattered) addend: bf16(bf16(x w^T) + addend).
Outputs are pre-filled with NaN, every launch runs twice (bit-stable), full-size addends also alias y.
Block level: MRLA_Bottleneck with functional.SHORTCUT_ADDEND on against off (the fill + scatter + torch add path): conv1's
backward node on the same incoming gradients, torch.equal on dx and its parameter gradients; two whole runs at the bounds
the suite already sets for two runs of one module; and the consumers that must still see true gradients."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _form(m, k, n):
    """Which kernel mrla_conv1x1_fwd[_addend] runs for x[m, k] w[n, k]^T, from the library's own queries."""
    from mrla_amd import _lib as L
    if L.load().mrla_conv1x1_add_supported(m, k, n, L.BF16) == 1:
        return "wide"
    if k <= 256:
        return "narrow"
    return "kstream256" if L.conv1x1_plan(m, k, n)[1] == 4 else "kstream"


def _scatter(addc, b, h, w, n, sh, sw):
    """The compact addend [b, hc, wc, n] in the output's pixels [b*h*w, n]: zeros elsewhere."""
    full = torch.zeros((b, h, w, n), dtype=addc.dtype, device=addc.device)
    full[:, ::sh, ::sw] = addc
    return full.reshape(b * h * w, n)


def _check(b, h, w, k, n, sh, sw, form, seed):
    from mrla_amd import _lib as L
    from tests.test_conv1x1_steady_gpu import _assert_bf16_close, _operands
    lib = L.load()
    m = b * h * w
    hc, wc = (h + sh - 1) // sh, (w + sw - 1) // sw
    assert _form(m, k, n) == form, (_form(m, k, n), form)
    assert lib.mrla_conv1x1_addend_supported(m, k, n, sh, sw, L.BF16) == 1
    x, wt = _operands(m, k, n, seed=seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    addc = torch.randn((b, hc, wc, n), device="cuda", generator=g).bfloat16()
    full = _scatter(addc, b, h, w, n, sh, sw)
    dense = sh == 1 and sw == 1

    def run(dst, addend):
        L.call("mrla_conv1x1_fwd_addend", _P(x), _P(wt), _P(addend), _P(dst), m, k, n, b, h, w, sh, sw, L.BF16, _stream())
        return dst
    nan = lambda: torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")  # noqa: E731
    y, y2 = run(nan(), addc), run(nan(), addc)
    want = nan()
    if form == "wide":
        L.call("mrla_conv1x1_fwd_add", _P(x), _P(wt), _P(full), _P(want), m, k, n, L.BF16, _stream())
    else:
        L.call("mrla_conv1x1_fwd", _P(x), _P(wt), _P(want), None, m, k, n, L.BF16, _stream())
        want = want + full
    torch.cuda.synchronize()
    assert torch.equal(y, y2), "two runs of the same launch differ"
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, want), f"{int((y != want).sum())} of {y.numel()} elements differ from the path it replaces"
    if dense:
        inplace = addc.reshape(m, n).clone()
        run(inplace, inplace)
        torch.cuda.synchronize()
        assert torch.equal(inplace, y), "in place (addend aliasing y) differs"
    if form == "wide":
        ref = x.double() @ wt.double().t()
        ref += full.double()
        _assert_bf16_close(y, ref, "y")


# (b, h, w, k, n, form): small maps -- odd ones, where ceil(h / s) matters, and ragged pixel counts (m % 32 != 0)
SMALL = [(3, 9, 9, 128, 256, "wide"), (2, 7, 5, 64, 512, "wide"), (4, 14, 14, 256, 256, "wide"), (5, 6, 10, 128, 512, "wide"),
         (3, 9, 9, 64, 64, "narrow"), (2, 7, 5, 128, 128, "narrow"), (4, 14, 14, 256, 64, "narrow"), (5, 6, 10, 64, 192, "narrow"),
         (3, 9, 9, 512, 1024, "kstream"), (2, 7, 5, 512, 128, "kstream"), (4, 14, 14, 1024, 384, "kstream"),
         (5, 6, 10, 2048, 256, "kstream")]


@pytest.mark.parametrize("stride", [(1, 1), (2, 2), (2, 1), (3, 2)], ids=lambda s: f"s{s[0]}{s[1]}")
@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_addend_forms_equal_the_paths_they_replace(case, stride):
    b, h, w, k, n, form = case
    _check(b, h, w, k, n, stride[0], stride[1], form, seed=5000 + h * w + k + n)


# one steady-state shape per form at the benchmark's batch (conv1's input gradient: k = planes, n = block input channels):
# stage 2 / 3 first blocks (wide, compact), stage 1 first block (narrow, full-size: a stride-1 downsample), stage 4 first
# block (K-streaming, compact), stage 4 blocks 2 - 3 (K-streaming, full-size), and the 256 x 256 tile form
STEADY = [(256, 56, 56, 128, 256, 2, "wide"), (256, 28, 28, 256, 512, 2, "wide"), (256, 56, 56, 64, 64, 1, "narrow"),
          (256, 14, 14, 512, 1024, 2, "kstream"), (256, 7, 7, 512, 2048, 1, "kstream"), (255, 7, 7, 512, 2048, 1, "kstream"),
          (256, 14, 14, 1024, 256, 2, "kstream256"), (256, 14, 14, 1024, 256, 1, "kstream256"),
          (255, 27, 28, 128, 256, 2, "wide"), (255, 55, 56, 64, 64, 2, "narrow")]


@pytest.mark.parametrize("case", STEADY, ids=lambda c: "x".join(map(str, c)))
def test_addend_forms_in_steady_state(case):
    from mrla_amd import _lib as L
    b, h, w, k, n, s, form = case
    m = b * h * w
    if form == "wide":                          # the LDS ring wraps: more units per workgroup than it is deep
        upw, depth, _, _ = L.conv1x1_plan(m, k, n, True)
        assert upw > depth, (upw, depth)
    elif form == "narrow":
        upw, depth, _, _ = L.conv1x1_plan(m, k, n)
        assert upw > depth, (upw, depth)
    else:
        chunks, stages, _, _ = L.conv1x1_plan(m, k, n)
        assert chunks >= 4 * stages
    _check(b, h, w, k, n, s, s, form, seed=6000 + k + n + s)


def test_addend_argument_validation():
    from mrla_amd import _lib as L
    lib = L.load()
    one = ctypes.c_void_p(16)
    # b * h * w != m, a zero stride: invalid, whatever the pointers say (nothing is launched)
    assert lib.mrla_conv1x1_fwd_addend(one, one, one, one, 100, 64, 256, 2, 7, 7, 2, 2, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_addend(one, one, one, one, 98, 64, 256, 2, 7, 7, 0, 2, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_addend(one, one, None, one, 98, 64, 256, 2, 7, 7, 2, 2, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_addend_supported(98, 64, 256, 0, 1, L.BF16) == L.EINVAL
    assert lib.mrla_conv1x1_addend_supported(98, 64, 256, 2, 2, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_addend_supported(98, 96, 256, 2, 2, L.BF16) == L.EUNSUPPORTED     # a reduction no GEMM takes
    for k, n in ((64, 256), (64, 64), (512, 2048)):                                            # all three families
        assert lib.mrla_conv1x1_addend_supported(98, k, n, 2, 2, L.BF16) == 1
    # the query of the wide form answers as before
    assert lib.mrla_conv1x1_add_supported(98, 64, 64, L.BF16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_add_supported(98, 512, 2048, L.BF16) == L.EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------
# block level
# ------------------------------------------------------------------------------------------------------
def _block(inplanes, planes, stride, seed):
    from mrla_amd import resnet
    torch.manual_seed(seed)
    ds = None
    if stride != 1 or inplanes != planes * 4:
        ds = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                 torch.nn.BatchNorm2d(planes * 4))
    blk = resnet.MRLA_Bottleneck(inplanes, planes, stride=stride, downsample=ds)
    for mod in blk.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(mod.weight, 0.6, 1.4)
            torch.nn.init.uniform_(mod.bias, -0.3, 0.3)
    return blk.cuda().to(memory_format=torch.channels_last).train()


def _run_block(blk, x, gup, on):
    from mrla_amd import functional as Fm
    old = Fm.SHORTCUT_ADDEND
    Fm.SHORTCUT_ADDEND = on
    try:
        blk.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = blk(xp)
        out.backward(gup)
        torch.cuda.synchronize()
    finally:
        Fm.SHORTCUT_ADDEND = old
    return out.detach().clone(), xp.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}


# (inplanes, planes, stride, map): the strided first block of stage 2 (wide form, compact addend), a stage-4 block
# (K-streaming, full-size), stage 4's strided first block (K-streaming, compact), stage 1's first block (narrow, full-size),
# and a strided block on an odd map (wide form, compact, ceil(27 / 2))
BLOCKS = [(256, 128, 2, 56), (2048, 512, 1, 7), (1024, 512, 2, 14), (64, 64, 1, 56), (512, 256, 2, 27)]


def _block_case(cfg):
    inplanes, planes, stride, hw = cfg
    b = 8
    blk = _block(inplanes, planes, stride, seed=11)
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.relu(torch.randn((b, inplanes, hw, hw), device="cuda", generator=g) + 0.3).bfloat16()
    x = x.contiguous(memory_format=torch.channels_last)
    ho = (hw + stride - 1) // stride
    gup = (torch.randn((b, planes * 4, ho, ho), device="cuda", generator=g) * 0.1).bfloat16()
    return blk, x, gup.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("cfg", BLOCKS, ids=lambda c: "x".join(map(str, c)))
def test_block_gradients_equal_the_fallback_path(cfg, monkeypatch):
    """MRLA_Bottleneck.forward as the model runs it; dx and the parameter gradients that conv1's backward node produces,
    with the shortcut addend inside the GEMM against the fallback path, torch.equal.

    Both paths must see THE SAME incoming gradients for a bit-for-bit comparison, and two runs of a whole block do not
    give them that: MIOpen's 3x3 convolution between conv1 and the block output is not run-to-run bit-stable at every
    shape (tests/test_block_bf16_gpu.py: "two calls of the same module differ in a few last bits"), so two backward passes
    of the same code already differ in dx.  So the block runs forward once, the part behind conv1 -- conv2, conv3, the
    downsample branch, the MRLA tail -- runs backward once, and the two gradients it delivers (to conv1's output and to the
    shortcut / the subsampled shortcut) go through conv1's node with SHORTCUT_ADDEND on, off and on again.  Everything in
    that node is this project's own kernels and torch's elementwise kernels, which are bit-stable.  Every other parameter
    gradient of the block is computed upstream of that node and does not depend on the path."""
    from mrla_amd import _lib as L, functional as Fm
    inplanes, planes, stride, hw = cfg
    blk, x, gup = _block_case(cfg)
    assert L.load().mrla_conv1x1_addend_supported(x.shape[0] * hw * hw, planes, inplanes, stride, stride, L.BF16) == 1
    assert (Fm.shortcut_subsample(blk.downsample, x) == (stride, stride)) == (stride != 1)
    seen = {}
    real = Fm.conv_bn_act

    def spy(*args, **kwargs):
        res = real(*args, **kwargs)
        if kwargs.get("passthrough"):
            seen["z1"], seen["ident"] = res
        return res
    monkeypatch.setattr(Fm, "conv_bn_act", spy)
    xp = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(xp)
    z1, ident = seen["z1"], seen["ident"]
    assert ident.grad_fn is not None                    # routed through conv1's node
    assert tuple(ident.shape[2:]) == ((hw + stride - 1) // stride,) * 2
    g_z1, g_ident = torch.autograd.grad(out, [z1, ident], gup, retain_graph=True)       # the rest of the block, once
    assert g_ident.shape == ident.shape                                                  # compact for the strided blocks
    leaves = [xp, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias]
    timer_names = ["mrla_conv1x1_bwd_data"]
    results = []
    for on in (True, False, True):
        monkeypatch.setattr(Fm, "SHORTCUT_ADDEND", on)
        Fm.TIMER = timer = Fm.KernelTimer(timer_names)
        try:
            results.append(torch.autograd.grad([z1, ident], leaves, [g_z1.clone(), g_ident.clone()], retain_graph=True))
            torch.cuda.synchronize()
        finally:
            Fm.TIMER = None
        assert len(timer.records) == 1                   # one input-gradient GEMM per backward on either path
    on1, off, on2 = results
    assert torch.isfinite(on1[0].float()).all() and on1[0].float().abs().max() > 0
    for name, a, b_, c in zip(("dx", "conv1.weight", "bn1.weight", "bn1.bias"), on1, off, on2):
        assert torch.equal(a, c), f"{name}: two runs differ"
        assert torch.equal(a, b_), f"{name}: {int((a != b_).sum())} of {a.numel()} elements differ from the fallback path"


@pytest.mark.parametrize("cfg", BLOCKS, ids=lambda c: "x".join(map(str, c)))
def test_whole_block_runs_agree_with_the_fallback_path(cfg):
    """Two complete forward + backward runs of the module, addend on and off.  Bounds: those tests/test_block_bf16_gpu.py
    sets for two runs of one module (MIOpen's 3x3 is not bit-stable everywhere): out beyond 2 bf16 ulps on < 1e-3 of the
    elements, dx on < 5e-2; parameter gradients to 1e-2 in relative L2 (tests/test_conv1x1_gpu.py)."""
    from tests.test_block_bf16_gpu import _ulps
    blk, x, gup = _block_case(cfg)
    out1, dx1, gr1 = _run_block(blk, x, gup, True)
    out0, dx0, gr0 = _run_block(blk, x, gup, False)
    assert torch.isfinite(dx1.float()).all() and dx1.float().abs().max() > 0
    f_out = (_ulps(out1, out0.double()) > 2.0).float().mean().item()
    f_dx = (_ulps(dx1, dx0.double()) > 2.0).float().mean().item()
    print(f"out beyond 2 ulps {f_out:.2e}, dx beyond 2 ulps {f_dx:.2e}")
    assert f_out < 1e-3 and f_dx < 5e-2
    assert gr1.keys() == gr0.keys() and len(gr1) > 10
    for name in gr1:
        den = gr0[name].float().norm().item()
        err = (gr1[name].float() - gr0[name].float()).norm().item() / max(den, 1e-30)
        assert err < 1e-2, (name, err)


def _pair(k=256, n=128, stride=2):
    conv = torch.nn.Conv2d(k, n, 1, bias=False).cuda().to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(n).cuda()
    return conv, bn


def _shortcut_case(x, conv, bn, sub, consume, on):
    """out, ident = conv_bn_act(x, ..., passthrough, subsample); `consume(ident)` -> scalar loss term; returns x.grad."""
    from mrla_amd import functional as Fm
    old = Fm.SHORTCUT_ADDEND
    Fm.SHORTCUT_ADDEND = on
    try:
        conv.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(True)
        out, ident = Fm.conv_bn_act(xp, conv, bn, relu=True, passthrough=True, subsample=sub)
        assert tuple(ident.shape[2:]) == ((x.shape[2] + sub[0] - 1) // sub[0], (x.shape[3] + sub[1] - 1) // sub[1])
        assert torch.equal(ident.detach(), x[:, :, ::sub[0], ::sub[1]])
        loss = (out.float() * out.float()).sum() + consume(ident)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        Fm.SHORTCUT_ADDEND = old
    return xp.grad.clone()


def test_other_consumers_of_the_subsampled_shortcut_see_true_gradients():
    """The subsampled shortcut is an ordinary output of conv1's autograd node: a second consumer, a tensor hook and
    torch.autograd.grad on it get the compact gradient itself, and the block input's gradient is conv1's input gradient plus
    ALL of it scattered -- whether the GEMM reads it compact or the fallback scatters it."""
    from mrla_amd import functional as Fm
    b, k, n, hw, sub = 4, 256, 128, 14, (2, 2)
    conv, bn = _pair(k, n)
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn((b, k, hw, hw), device="cuda", generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    c1 = torch.randn((b, k, 7, 7), device="cuda", generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    c2 = torch.randn((b, k, 7, 7), device="cuda", generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    base = _shortcut_case(x, conv, bn, sub, lambda t: (t * 0).sum(), True)         # conv1's own input gradient (+ zeros)

    def close(got, gc):                      # bf16 dX + scattered compact gradient.  The wide form rounds their fp32 sum
        full = torch.zeros_like(x)           # once; this restatement starts from the rounded dX: half an ulp of each term
        full[:, :, ::2, ::2] = gc
        want = base.float() + full.float()
        return ((got.float() - want).abs() <= (base.float().abs() + want.abs()) * 2.0 ** -8 + 1e-30).all()

    # (a) two consumers: autograd sums their compact gradients in front of conv1's node
    two = lambda t: (t * c1).sum() + (t.float() * c2.float()).sum()                # noqa: E731
    got_on, got_off = _shortcut_case(x, conv, bn, sub, two, True), _shortcut_case(x, conv, bn, sub, two, False)
    assert torch.equal(got_on, got_off)
    assert close(got_on, (c1.float() + c2.float()).bfloat16())
    # (b) a hook on it sees the compact gradient, and may edit it
    seen = {}

    def hooked(t):
        t.register_hook(lambda gr: seen.__setitem__("g", gr.detach().clone()))
        return (t * c1).sum()
    got_on, got_off = _shortcut_case(x, conv, bn, sub, hooked, True), _shortcut_case(x, conv, bn, sub, hooked, False)
    assert torch.equal(seen["g"], c1) and torch.equal(got_on, got_off)
    assert close(got_on, c1)
    # (c) torch.autograd.grad with respect to it: the compact gradient, not a placeholder
    xp = x.clone().requires_grad_(True)
    out, ident = Fm.conv_bn_act(xp, conv, bn, relu=True, passthrough=True, subsample=sub)
    gi, = torch.autograd.grad((ident * c1).sum() + out.float().sum(), ident)
    assert torch.equal(gi, c1)
    # (d) only the shortcut carries a gradient
    xp = x.clone().requires_grad_(True)
    out, ident = Fm.conv_bn_act(xp, conv, bn, relu=True, passthrough=True, subsample=sub)
    (ident * c1).sum().backward()
    full = torch.zeros_like(x)
    full[:, :, ::2, ::2] = c1
    assert torch.equal(xp.grad, full)


def test_inputs_off_the_gemm_path_keep_the_dense_gradient():
    """fp32 / NCHW inputs and channel counts no GEMM takes: shortcut_subsample() declines or conv1 runs the stock
    convolution; the subsample is then _SubsampleFn's, whose backward scatters into zeros, and autograd accumulates."""
    from mrla_amd import functional as Fm
    b, k, hw = 2, 256, 14
    ds = torch.nn.Sequential(torch.nn.Conv2d(k, 512, 1, stride=2, bias=False), torch.nn.BatchNorm2d(512)).cuda()
    x32 = torch.randn((b, k, hw, hw), device="cuda")
    assert Fm.shortcut_subsample(ds, x32) is None                                            # fp32, NCHW
    assert Fm.shortcut_subsample(ds, x32.bfloat16()) is None                                 # bf16, NCHW
    xcl = x32.bfloat16().contiguous(memory_format=torch.channels_last)
    assert Fm.shortcut_subsample(ds, xcl) == (2, 2)
    assert Fm.shortcut_subsample(ds[0], xcl) is None and Fm.shortcut_subsample(None, xcl) is None
    # conv1 with 96 output channels runs the stock convolution: the second result is still the subsample, dense backward
    conv, bn = torch.nn.Conv2d(k, 96, 1, bias=False).cuda().to(memory_format=torch.channels_last), torch.nn.BatchNorm2d(96).cuda()
    c1 = torch.randn((b, k, 7, 7), device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    xp = xcl.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, ident = Fm.conv_bn_act(xp, conv, bn, relu=True, passthrough=True, subsample=(2, 2))
    assert torch.equal(ident.detach(), xcl[:, :, ::2, ::2])
    (ident * c1).sum().backward()
    full = torch.zeros_like(xcl)
    full[:, :, ::2, ::2] = c1
    assert torch.equal(xp.grad, full)
