"""GPU: the 1x1 GEMMs with an eval-mode BatchNorm (+ReLU) folded into their store (mrla_conv1x1_fwd_affine;
resnet_mrla_light.py:93-94 `conv1 -> bn1 -> relu` and :196-199, the downsample branch, under model.eval(); mmdet's
resnet_mrlal.py:358-367 for the frozen first stage of the detection backbone).

The contract is bit-equality with the two launches the fold replaces -- mrla_conv1x1_fwd into a temporary, then
mrla_bn_act_fwd(..., MRLA_NHWC) -- so every comparison here is torch.equal on int16 views, never a tolerance:
  1. the C ABI against the two launches, per kernel form and element type (the forms are asserted from the planner);
  2. functional.conv_bn_act takes the folded route exactly where nothing will be differentiated, and nowhere else;
  3. whole models with functional.EVAL_FOLD on and off;
  4. one HIP-graph capture of the folded inference forward."""
import contextlib
import ctypes
import functools
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    """The stock convolutions beside the GEMMs (the strided 3x3 of a stage's first block is the first one in resnet50_mrlal)
    get MIOpen solvers that accumulate atomically unless told otherwise: two launches of the SAME forward then differ in the
    last bits, and bit-equality between two routes would say nothing about the routes.  With deterministic solvers only, and
    one warm-up call per route (MIOpen's first call of a problem may take another solver than the later ones), it does."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ldt(dtype):
    from mrla_amd import _lib as L
    return L.BF16 if dtype == torch.bfloat16 else L.F16


def _bits(t):
    return t.view(torch.int16)


# ---- 1. the C ABI against the two launches ---------------------------------------------------------------------------------
# (m, k, n) -> the kernel form the planner must pick: the kernels can only go wrong per form.  m = 98 = 2*7*7 (ragged: one
# partial 32-pixel block); "steady": a workgroup / pixel-wave walks more blocks than its pipeline is deep.
SHAPES = [
    ((98, 64, 64), "narrow"), ((98, 128, 128), "narrow"), ((98, 256, 64), "narrow"), ((98, 256, 128), "narrow"),
    ((98, 64, 192), "narrow"),
    ((200704, 64, 64), "narrow-steady"),
    ((200704, 256, 64), "narrow"),               # (two blocks per pixel-wave: as deep as the prefetch, not deeper)
    ((270000, 256, 64), "narrow-steady"),        # (200704 pixels give an eight-wave workgroup's pixel-waves 2 blocks each: not
    #                                               more than the prefetch depth.  270000 = 8437.5 blocks: 3 each, ragged too)
    ((98, 64, 256), "wide"), ((98, 128, 512), "wide"), ((98, 256, 1024), "wide"),
    ((200704, 64, 256), "wide-steady"), ((50176, 256, 1024), "wide-steady"),
    ((98, 512, 128), "ks<2,1>"),                 # (one tile either way; (200, ...) below tells <2,1> from <2,2>)
    ((200, 512, 128), "ks<2,1>"),
    ((98, 512, 256), "ks<4,1>"),
    ((76700, 512, 128), "ks<2,2>"), ((38300, 512, 256), "ks<4,2>"),
    ((20300, 1024, 512), "ks<4,2>"),             # (160 tiles of 256 x 256 would not fill 70 % of a round: the 128 x 256 tiles)
    ((22900, 1024, 512), "ks256"),               # (20300 pixels are 160 tiles of 256 x 256, under the planner's 70 % of a round
    #                                               of 256 workgroups: the smaller tiles.  22900: 180 tiles, ragged last one)
]


def _assert_form(m, k, n, form, dt):
    from mrla_amd import _lib as L
    plan = L.conv1x1_plan(m, k, n, False, dt)
    assert plan is not None, (m, k, n)
    upw, depth, wgs, rows = plan
    assert rows == L.load().mrla_conv1x1_rows(m, k, n, dt)
    if form.startswith("narrow"):
        assert wgs > 0 and depth == 2 and not (n % 256 == 0), plan
    elif form.startswith("wide"):
        assert wgs > 0 and n % 256 == 0 and depth == {64: 16, 128: 8, 256: 5}[k], plan
    elif form == "ks256":
        assert wgs == 0 and depth == 4 and upw == k // 32 and rows == -(-m // 256), plan
        assert m % 256 and rows * (n // 256) >= 160
    else:
        wn, pb = int(form[3]), int(form[5])
        tm = (8 // wn) * pb * 32                               # pixels of a tile: one record row per tile
        assert wgs == 0 and depth == 3 and upw == k // 32 and rows == -(-m // tm), (plan, tm)
        assert (n % 256 == 0) == (wn == 4)
    if form.endswith("steady"):
        assert upw > depth, plan


@functools.lru_cache(maxsize=1)
def _problem(shape, dname):
    """Operands, coefficients and the two-launch reference for both `relu` values: built once per shape and element type."""
    from mrla_amd import _lib as L
    m, k, n = shape
    dtype, dt = TDT[dname], _ldt(TDT[dname])
    g = torch.Generator(device="cuda").manual_seed(1000003 * k + 1009 * n + m)
    x = torch.randn((m, k), device="cuda", generator=g).to(dtype)
    w = (torch.randn((n, k), device="cuda", generator=g) / k ** 0.5).to(dtype)
    # x w^T ~ N(0, 1) per output.  sc: both signs, |sc| in [0.5, 2], one channel exactly 0; sh small against sc * y, so that
    # about half of the outputs are negative and the ReLU bites under either sign of sc
    sc = (0.5 + 1.5 * torch.rand((n,), device="cuda", generator=g)) * (1 - 2.0 * (torch.rand((n,), device="cuda", generator=g) < 0.5))
    sc[n // 3] = 0.0
    sh = torch.rand((n,), device="cuda", generator=g) - 0.5
    z = torch.full((m, n), float("nan"), dtype=dtype, device="cuda")
    L.call("mrla_conv1x1_fwd", _P(x), _P(w), _P(z), None, m, k, n, dt, _stream())
    ref = []
    for relu in (0, 1):
        y = torch.full((m, n), float("nan"), dtype=dtype, device="cuda")
        L.call("mrla_bn_act_fwd", _P(z), _P(sc), _P(sh), relu, _P(y), 1, n, m, 1, dt, L.NHWC, _stream())
        ref.append(y)
    torch.cuda.synchronize()
    neg = (ref[0].float() < 0).float().mean().item()
    assert 0.3 < neg < 0.7 and torch.isfinite(ref[0].float()).all(), neg
    assert (ref[1][:, n // 3].float() == max(sh[n // 3].to(dtype).float().item(), 0.0)).all()     # the sc = 0 channel: relu?(sh)
    return x, w, sc, sh, ref


@pytest.mark.parametrize("relu", [0, 1], ids=["affine", "relu"])
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("shape, form", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_bit_equal_to_the_two_launches(shape, form, dname, relu):
    from mrla_amd import _lib as L
    m, k, n = shape
    dtype, dt = TDT[dname], _ldt(TDT[dname])
    assert L.load().mrla_conv1x1_fwd_affine_supported(m, k, n, dt) == 1
    _assert_form(m, k, n, form, dt)
    x, w, sc, sh, ref = _problem(shape, dname)
    guard = 40                                             # rows behind the m-th: never written, whatever the tile height
    outs = []
    for _ in range(2):
        y = torch.full((m + guard, n), float("nan"), dtype=dtype, device="cuda")
        _bits(y).fill_(0x7fc1 if dtype == torch.bfloat16 else 0x7e01)         # a NaN with a payload: the poison
        L.call("mrla_conv1x1_fwd_affine", _P(x), _P(w), _P(sc), _P(sh), relu, _P(y), m, k, n, dt, _stream())
        outs.append(y)
    torch.cuda.synchronize()
    poison = outs[0].new_empty((guard, n))
    _bits(poison).fill_(0x7fc1 if dtype == torch.bfloat16 else 0x7e01)
    for y in outs:
        assert torch.equal(_bits(y[m:]), _bits(poison)), "rows past m were written"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs of the same launch differ"
    got, want = _bits(outs[0][:m]), _bits(ref[relu])
    if not torch.equal(got, want):
        bad = (got != want)
        rows_, cols_ = bad.nonzero(as_tuple=True)
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ from the two launches; first at "
                             f"({int(rows_[0])}, {int(cols_[0])}): {outs[0][rows_[0], cols_[0]].item()} vs "
                             f"{ref[relu][rows_[0], cols_[0]].item()}; rows {int(rows_.min())}..{int(rows_.max())}, "
                             f"columns {int(cols_.min())}..{int(cols_.max())}")


def test_misaligned_coefficients_are_refused_on_the_host():
    from mrla_amd import _lib as L
    x = torch.zeros((98, 64), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((64, 64), dtype=torch.bfloat16, device="cuda")
    y = torch.zeros((98, 64), dtype=torch.bfloat16, device="cuda")
    c = torch.zeros((2, 68), dtype=torch.float32, device="cuda")
    rc = L.load().mrla_conv1x1_fwd_affine(_P(x), _P(w), _P(c[0][1:]), _P(c[1]), 1, _P(y), 98, 64, 64, L.BF16, _stream())
    assert rc == L.EINVAL


# ---- 2. routing through functional.conv_bn_act ---------------------------------------------------------------------------
@contextlib.contextmanager
def _logged(fold):
    """functional.EVAL_FOLD = fold, and the names of the C calls made inside."""
    from mrla_amd import _lib as L, functional as Fm
    names, orig, was = [], L.call, Fm.EVAL_FOLD
    L.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    Fm.EVAL_FOLD = fold
    try:
        yield names
        torch.cuda.synchronize()
    finally:
        L.call, Fm.EVAL_FOLD = orig, was


def _pair(k, n, stride, dtype, w16, seed):
    """A 1x1 convolution and its BatchNorm with non-trivial running statistics; w16: the weight in `dtype`, else fp32."""
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(k, n, 1, stride=stride, bias=False).cuda().to(memory_format=CL)
    bn = torch.nn.BatchNorm2d(n).cuda()
    with torch.no_grad():
        bn.weight.uniform_(-1.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
    if w16:
        conv = conv.to(dtype)
    return conv, bn.eval()


def _input(b, k, h, w, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((b, k, h, w), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)


def _amp(dtype, w16):
    """fp32 weights run under autocast, 16-bit ones without."""
    return contextlib.nullcontext() if w16 else torch.autocast("cuda", dtype=dtype)


FOLD_CASES = {
    # name: (b, k, h, w, n, stride, relu, passthrough, subsample, grad mode)
    "conv1-relu-no_grad": (2, 256, 14, 14, 64, 1, True, False, None, False),
    "strided-downsample-odd-map": (2, 256, 15, 15, 512, 2, False, False, None, False),
    "passthrough-with-subsample": (2, 256, 14, 14, 128, 1, True, True, (2, 2), False),
    "frozen-in-grad-mode": (2, 64, 14, 14, 64, 1, True, False, None, True),
}


@pytest.mark.parametrize("w16", [False, True], ids=["fp32-weights-autocast", "16-bit-weights"])
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(FOLD_CASES))
def test_conv_bn_act_folds_where_nothing_is_differentiated(case, dname, w16):
    from mrla_amd import functional as Fm
    b, k, h, w, n, stride, relu, passthrough, sub, grad = FOLD_CASES[case]
    dtype = TDT[dname]
    conv, bn = _pair(k, n, stride, dtype, w16, seed=11)
    if grad:                                   # the detection backbone's frozen stage: grad mode on, every tensor frozen
        for p in list(conv.parameters()) + list(bn.parameters()):
            p.requires_grad_(False)
    x = _input(b, k, h, w, dtype, seed=12)
    # the strided downsample runs on the GEMMs in bf16 only (functional.conv1x1_applies): in fp16 it keeps its stock
    # convolution, and there is nothing to fold
    folds = not (stride != 1 and dtype == torch.float16)
    res = {}
    for fold in (False, True, False):          # (the first: MIOpen's warm-up, where a stock convolution takes part)
        with _logged(fold) as names, torch.set_grad_enabled(grad), _amp(dtype, w16):
            out = Fm.conv_bn_act(x, conv, bn, relu=relu, passthrough=passthrough, subsample=sub)
        res[fold] = (out, list(names))
    out_on, names_on = res[True]
    out_off, names_off = res[False]
    if passthrough:
        (out_on, thr_on), (out_off, thr_off) = out_on, out_off
        assert torch.equal(thr_on, x[:, :, ::2, ::2]) and torch.equal(thr_off, thr_on)
        assert thr_on.is_contiguous(memory_format=CL)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    assert out_on.shape == (b, n, ho, wo) and out_on.dtype == dtype and out_on.is_contiguous(memory_format=CL)
    assert out_on.grad_fn is None and not out_on.requires_grad
    assert torch.equal(_bits(out_on), _bits(out_off)), "EVAL_FOLD changes the values"
    assert torch.isfinite(out_on.float()).all() and out_on.float().abs().max() > 0
    assert "mrla_conv1x1_fwd_affine" not in names_off
    if folds:
        assert names_on.count("mrla_conv1x1_fwd_affine") == 1, names_on
        assert not {"mrla_bn_act_fwd", "mrla_bn_fwd", "mrla_conv1x1_fwd"} & set(names_on), names_on
        assert "mrla_conv1x1_fwd" in names_off and {"mrla_bn_act_fwd", "mrla_bn_fwd"} & set(names_off), names_off
    else:
        assert names_on == names_off and "mrla_conv1x1_fwd_affine" not in names_on


def test_half_precision_running_statistics_keep_working():
    """model.half(): running_mean / running_var arrive as fp16 buffers and go through _RunningStats' fp32 copies."""
    from mrla_amd import functional as Fm
    conv, bn = _pair(256, 64, 1, torch.float16, True, seed=13)
    bn = bn.half()
    x = _input(2, 256, 14, 14, torch.float16, seed=14)
    before = (bn.running_mean.clone(), bn.running_var.clone())
    res = {}
    for fold in (True, False):
        with _logged(fold) as names, torch.no_grad():
            res[fold] = (Fm.conv_bn_act(x, conv, bn, relu=True), list(names))
    assert "mrla_conv1x1_fwd_affine" in res[True][1]
    assert torch.equal(_bits(res[True][0]), _bits(res[False][0]))
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])


@pytest.mark.parametrize("case", ["bn-train", "defer", "weight-requires-grad", "fp32-input"])
def test_conv_bn_act_keeps_its_route_where_a_backward_may_follow(case):
    from mrla_amd import functional as Fm
    dtype = torch.float32 if case == "fp32-input" else torch.bfloat16
    conv, bn = _pair(256, 64, 1, dtype, False, seed=15)
    if case == "bn-train":
        bn.train()
    x = _input(2, 256, 14, 14, dtype, seed=16)
    if case != "weight-requires-grad":
        x.requires_grad_(True)
    else:
        assert conv.weight.requires_grad and not x.requires_grad
    amp = contextlib.nullcontext() if dtype == torch.float32 else torch.autocast("cuda", dtype=dtype)
    with _logged(True) as names, amp:
        out = Fm.conv_bn_act(x, conv, bn, relu=case != "defer", defer=case == "defer")
        names = list(names)
    assert "mrla_conv1x1_fwd_affine" not in names, names
    if case == "fp32-input":                  # the stock convolution, then the BatchNorm passes
        assert "mrla_conv1x1_fwd" not in names and "mrla_bn_fwd" in names, names
    else:
        assert "mrla_conv1x1_fwd" in names and {"mrla_bn_fwd", "mrla_bn_act_fwd", "mrla_bn_stats_fwd_rows"} & set(names), names
    if case == "defer":
        assert hasattr(out, "_mrla_affine")
    assert out.grad_fn is not None
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    assert conv.weight.grad is not None and torch.isfinite(conv.weight.grad).all()
    if case != "weight-requires-grad":
        assert x.grad is not None and torch.isfinite(x.grad.float()).all() and x.grad.float().abs().max() > 0


# ---- 3. models ---------------------------------------------------------------------------------------------------------------
def _quiet(make):
    with contextlib.redirect_stdout(io.StringIO()):
        return make()


def _randomize_bn(net, seed):
    """Fresh networks have bn3.weight = 0 and unit statistics: give every BatchNorm an affine worth folding."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, device="cuda", generator=g))
                m.bias.copy_(0.2 * (torch.rand(m.bias.shape, device="cuda", generator=g) - 0.5))
                m.running_mean.copy_(0.2 * (torch.rand(m.bias.shape, device="cuda", generator=g) - 0.5))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, device="cuda", generator=g))


def _foldable_pairs(net, x, stages=None):
    """conv1 -> bn1 and downsample pairs of the bottlenecks (of `stages`) whose GEMM shape mrla_conv1x1_rows accepts, counted
    from the shapes the blocks actually see."""
    from mrla_amd import _lib as L
    from mrla_amd.resnet import _BottleneckTrunk
    seen, hooks = [], []
    for name, mod in net.named_modules():
        if isinstance(mod, _BottleneckTrunk) and (stages is None or name.split(".")[0] in stages):
            hooks.append(mod.register_forward_pre_hook(lambda m_, a: seen.append((m_, tuple(a[0].shape)))))
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            net(x)
    finally:
        for h in hooks:
            h.remove()
    lib, count = L.load(), 0
    for mod, (b, c, h, w) in seen:
        count += lib.mrla_conv1x1_rows(b * h * w, c, mod.conv1.out_channels, L.BF16) >= 0
        if mod.downsample is not None:
            s = mod.downsample[0].stride[0]
            count += lib.mrla_conv1x1_rows(b * ((h + s - 1) // s) * ((w + s - 1) // s), c, mod.downsample[0].out_channels, L.BF16) >= 0
    return count


@functools.lru_cache(maxsize=1)
def _classifier():
    from mrla_amd import models
    net = _quiet(models.resnet50_mrlal).cuda().eval()
    _randomize_bn(net, 21)
    x = torch.randn((2, 3, 224, 224), device="cuda", generator=torch.Generator(device="cuda").manual_seed(22))
    return net, x


def test_resnet50_inference_is_bit_equal_and_folds_every_eligible_pair():
    net, x = _classifier()
    want = _foldable_pairs(net, x)
    assert want == 20                              # 16 conv1 -> bn1 -> relu pairs and 4 downsample pairs at 224 x 224
    res = {}
    for key, fold in (("warm-up", False), ("on", True), ("off", False), ("on again", True)):
        with _logged(fold) as names, torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            res[key] = (net(x).clone(), list(names))
    assert res["on"][1].count("mrla_conv1x1_fwd_affine") == want and "mrla_conv1x1_fwd_affine" not in res["off"][1]
    assert torch.isfinite(res["on"][0].float()).all()
    assert torch.equal(res["on"][0], res["on again"][0]), "the forward does not reproduce itself: the comparison below says nothing"
    assert torch.equal(res["on"][0], res["off"][0]), "EVAL_FOLD changes the logits"


def test_detection_backbone_folds_its_frozen_stage_only():
    from mrla_amd import mmdet_backbone as mb
    net = _quiet(lambda: mb.ResNet_mrlal(frozen_stages=1, norm_eval=True)).cuda()
    _randomize_bn(net, 23)
    net.train()
    x = torch.randn((2, 3, 64, 96), device="cuda", generator=torch.Generator(device="cuda").manual_seed(24))
    assert _foldable_pairs(net, x, stages=("layer1",)) == 4        # 3 conv1 pairs and layer1's downsample
    res = {}
    for fold in (False, True, False):          # (the first: MIOpen's warm-up)
        net.zero_grad(set_to_none=True)
        with _logged(fold) as names, torch.autocast("cuda", dtype=torch.bfloat16):
            maps = net(x)
            names = list(names)
        sum(m.float().square().mean() for m in maps).backward()     # a backward pass runs through the unfrozen stages
        torch.cuda.synchronize()
        grads = [p.grad for p in net.layer2.parameters() if p.requires_grad]
        assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
        assert all(p.grad is None for p in net.layer1.parameters())
        res[fold] = ([m.detach() for m in maps], names)
    assert res[True][1].count("mrla_conv1x1_fwd_affine") == 4 and "mrla_conv1x1_fwd_affine" not in res[False][1]
    assert len(res[True][0]) == 4
    for a, b_ in zip(res[True][0], res[False][0]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b_), "EVAL_FOLD changes an output map"


# ---- 4. one graph capture -----------------------------------------------------------------------------------------------------
def test_folded_inference_forward_replays_from_a_graph():
    net, x = _classifier()

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return net(x)
    fwd()                                          # (MIOpen's warm-up)
    with _logged(True) as names:
        eager = fwd().clone()
    assert "mrla_conv1x1_fwd_affine" in names
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with _logged(True) as names, torch.cuda.graph(graph):
        out = fwd()
    assert names.count("mrla_conv1x1_fwd_affine") == 20
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "a replay differs from the eager forward"
