"""mrla_conv1x1_wgrad_bn: the BatchNorm backward apply dy = e*dz + f*xb + h formed inside the weight-gradient GEMM
(mrla_amd/csrc/conv1x1_wgrad.hip), and the one autograd node that brings a convolution + BatchNorm pair there
(functional._ConvBnFn; reference call sites resnet_mrla_light.py:93-94, 100-101, 196-199).

Kernel level, through the C ABI: the fused launch against mrla_bn_act_bwd followed by mrla_conv1x1_wgrad ON THE SAME
INPUTS, bit for bit (torch.equal) on dy_out, on the partial tiles the plan says are written, and on dw.  Outputs are
pre-filled with NaN.  Every case asserts the pipeline situation it is there for from mrla_conv1x1_wgrad_plan.
Module level: conv_bn_act with functional.WGRAD_BN on against off, torch.equal on dx, dW, dgamma, dbeta."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

_TD = {"bf16": torch.bfloat16, "f16": torch.float16}


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _situation(m, k, n, dt):
    """(chunks per workgroup as 'one' / 'few' / 'many', whether the last workgroup's range ends short, (tile n, tile k),
    splits) from the library's own plan."""
    from mrla_amd import _lib as L
    cpw, stages, tn, tk, splits, tiles = L.conv1x1_wgrad_plan(m, k, n, dt)
    chunks = (m + 31) // 32
    kind = "one" if cpw == 1 else "few" if 2 <= cpw <= stages else "many" if cpw > stages + 1 else "edge"
    return kind, chunks < cpw * splits, (tn, tk), splits, tiles


def _check(m, k, n, dtype, relu, dw32, seed):
    from mrla_amd import _lib as L
    lib = L.load()
    td, dt = _TD[dtype], (L.BF16 if dtype == "bf16" else L.F16)
    assert lib.mrla_conv1x1_wgrad_bn_supported(m, k, n, dt) == 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)       # noqa: E731
    g, xb, x = rnd(m, n).to(td), rnd(m, n).to(td), rnd(m, k).to(td)
    sc = torch.rand((n,), device="cuda", generator=gen) + 0.5
    sc[::7] = 0.0                                        # bn3's zero-initialised scale: z = sh, the mask is per channel
    sc[3::11] *= -1.0
    sh = rnd(n) * 0.5
    cb = torch.stack([torch.rand((n,), device="cuda", generator=gen) + 0.5, rnd(n) * 0.25,
                      rnd(n) * 0.1 + 300.0], dim=1).contiguous()      # a large h: a row past M that leaked would show
    wdt, wtd = (L.F32, torch.float32) if dw32 else (dt, td)
    rows = lib.mrla_conv1x1_wgrad_rows(m, k, n, dt)
    _, _, _, splits, _ = _situation(m, k, n, dt)
    assert rows == splits

    def bufs():
        return (torch.full((m, n), float("nan"), dtype=td, device="cuda"),
                torch.full((rows, n, k), float("nan"), dtype=torch.float32, device="cuda"),
                torch.full((n, k), float("nan"), dtype=wtd, device="cuda"))
    dy0, part0, dw0 = bufs()
    L.call("mrla_bn_act_bwd", _P(g), _P(xb), _P(sc), _P(sh), _P(cb), relu, _P(dy0), 1, n, m, 1, dt, L.NHWC, _stream())
    L.call("mrla_conv1x1_wgrad", _P(dy0), _P(x), _P(part0), _P(dw0), m, k, n, dt, wdt, _stream())
    dy1, part1, dw1 = bufs()
    L.call("mrla_conv1x1_wgrad_bn", _P(g), _P(xb), _P(sc), _P(sh), _P(cb), relu, _P(dy1), _P(x), _P(part1), _P(dw1),
           m, k, n, dt, wdt, _stream())
    torch.cuda.synchronize()
    assert torch.isfinite(dy0.float()).all() and torch.isfinite(part0).all() and torch.isfinite(dw0.float()).all()
    assert dy0.float().abs().max() > 100                 # h arrived
    assert torch.equal(dy1, dy0), f"dy_out: {int((dy1 != dy0).sum())} of {dy0.numel()} elements differ"
    assert torch.equal(part1, part0), f"part: {int((part1 != part0).sum())} of {part0.numel()} elements differ"
    assert torch.equal(dw1, dw0), f"dw: {int((dw1 != dw0).sum())} of {dw0.numel()} elements differ"


KN = [(k, n) for k in (64, 128, 256) for n in (64, 128, 256)]


def test_the_small_cases_cover_all_eight_tile_shapes():
    from mrla_amd import _lib as L
    tiles = {_situation(1000, k, n, L.BF16)[2] for k, n in KN}
    assert tiles == {(64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (128, 256), (256, 64), (256, 128)}


@pytest.mark.parametrize("dw32", [0, 1], ids=["dw16", "dw32"])
@pytest.mark.parametrize("relu", [0, 1], ids=["lin", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kn", KN, ids=lambda c: f"k{c[0]}n{c[1]}")
def test_every_tile_shape_one_ragged_chunk_per_workgroup(kn, dtype, relu, dw32):
    from mrla_amd import _lib as L
    k, n = kn
    kind, _, _, _, _ = _situation(1000, k, n, L.BF16)
    assert kind == "one" and 1000 % 32 != 0
    _check(1000, k, n, dtype, relu, dw32, seed=7000 + k + 3 * n + relu)


# (m, k, n, chunks per workgroup, last range short, k-tiles > 1, n-tiles > 1)
DEEP = [(4100, 512, 256, "few", False, True, True), (4100, 256, 1024, "edge", True, False, True),
        (50000, 64, 64, "many", True, False, False), (4100, 64, 64, "one", False, False, False)]


@pytest.mark.parametrize("relu", [0, 1], ids=["lin", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", DEEP, ids=lambda c: f"m{c[0]}k{c[1]}n{c[2]}")
def test_tiled_and_deep_pipelines(case, dtype, relu):
    from mrla_amd import _lib as L
    m, k, n, kind, short, ktiles, ntiles = case
    got_kind, got_short, (tn, tk), _, tiles = _situation(m, k, n, L.BF16)
    assert (got_kind, got_short) == (kind, short), (got_kind, got_short)
    assert (k // tk > 1) == ktiles and (n // tn > 1) == ntiles and tiles == (k // tk) * (n // tn)
    # (fp16 dw only where it cannot overflow: thousands of pixels of |dy| ~ h = 300 sum past 65504)
    _check(m, k, n, dtype, relu, dw32=1 if dtype == "f16" else relu, seed=8000 + k + n + relu)


def test_the_deep_cases_cover_every_pipeline_situation():
    kinds = {c[3] for c in DEEP}
    assert {"one", "few", "many"} <= kinds and any(c[4] for c in DEEP) and any(c[5] for c in DEEP) and any(c[6] for c in DEEP)


# ------------------------------------------------------------------------------------------------------
# module level
# ------------------------------------------------------------------------------------------------------
def _pair(k=64, n=256, stride=1, seed=3):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(k, n, 1, stride=stride, bias=False).cuda().to(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(n).cuda()
    torch.nn.init.uniform_(bn.weight, 0.6, 1.4)
    torch.nn.init.uniform_(bn.bias, -0.3, 0.3)
    return conv, bn


def _inputs(k=64, n=256, hw=8, stride=1, seed=4):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((2, k, hw, hw), device="cuda", generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    ho = (hw + stride - 1) // stride
    gup = torch.randn((2, n, ho, ho), device="cuda", generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    return x, gup


class _recorded:
    """Every C-ABI entry the library is asked for inside the block, as (name, args), in order (functional._call and
    the sequence entry points both go through _lib.call)."""

    def __enter__(self):
        from mrla_amd import _lib as L
        self.calls, self._call = [], L.call
        L.call = lambda name, *a: (self.calls.append((name, a)), self._call(name, *a))[1]
        return self.calls

    def __exit__(self, *exc):
        from mrla_amd import _lib as L
        L.call = self._call


def _assert_route(calls, route, wgrad=True):
    """route 'fused': the backward launched mrla_conv1x1_wgrad_bn and neither an apply pass nor the plain weight gradient;
    'two_pass': the reverse (wgrad=False: a frozen weight, no weight gradient at all).  The apply pass is mrla_bn_act_bwd
    or, on the sequence route, mrla_bn_bwd with a dx (argument 10); dx = NULL there means the sums and constants only."""
    names = [n for n, _ in calls]
    seq = [a for n, a in calls if n == "mrla_bn_bwd"]
    applies = "mrla_bn_act_bwd" in names or any(a[10] is not None for a in seq)
    if route == "fused":
        assert names.count("mrla_conv1x1_wgrad_bn") >= 1, names
        assert "mrla_conv1x1_wgrad" not in names and not applies, names
        assert (seq and all(a[10] is None for a in seq)) or "mrla_bn_stats_bwd" in names, names
    else:
        assert "mrla_conv1x1_wgrad_bn" not in names and applies, names
        assert ("mrla_conv1x1_wgrad" in names) == wgrad, names


def _run(conv, bn, x, gup, on, relu=True, defer=False, loss=None, fused_expected=None, route=None, wgrad=True):
    """One forward + backward of conv_bn_act with WGRAD_BN = on; (dx, dW, dgamma, dbeta, out, calls).  The entry points
    the backward asked for are held to `route` (default: 'fused' with WGRAD_BN on, 'two_pass' with it off)."""
    from mrla_amd import functional as Fm
    old = Fm.WGRAD_BN
    Fm.WGRAD_BN = on
    rec = _recorded()
    try:
        calls = rec.__enter__()
        conv.zero_grad(set_to_none=True)
        bn.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(True)
        out = Fm.conv_bn_act(xp, conv, bn, relu=relu, defer=defer)
        is_fused = "_ConvBnFn" in type(out.grad_fn).__name__
        assert is_fused == (on if fused_expected is None else fused_expected), type(out.grad_fn).__name__
        if loss is None:
            out.backward(gup)
        else:
            loss(out).backward()
        torch.cuda.synchronize()
    finally:
        rec.__exit__()
        Fm.WGRAD_BN = old
    if route != "any":
        _assert_route(calls, route or ("fused" if on else "two_pass"), wgrad)
    wg = conv.weight.grad.clone() if conv.weight.grad is not None else None
    return xp.grad.clone(), wg, bn.weight.grad.clone(), bn.bias.grad.clone(), out.detach().clone(), calls


def _same(a, b):
    for name, u, v in zip(("dx", "dW", "dgamma", "dbeta", "out"), a, b):
        assert torch.isfinite(u.float()).all(), name
        assert torch.equal(u, v), f"{name}: {int((u != v).sum())} of {u.numel()} elements differ"
    assert a[0].float().abs().max() > 0 and a[1].float().abs().max() > 0


@pytest.mark.parametrize("form", ["relu", "linear", "deferred", "strided"])
def test_one_node_equals_two_nodes(form):
    stride = 2 if form == "strided" else 1
    conv, bn = _pair(stride=stride)
    x, gup = _inputs(hw=16 if stride == 2 else 8, stride=stride)
    kw = dict(relu=form in ("relu", "strided"), defer=form == "deferred")
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, **kw)
    bn.load_state_dict(state)
    b = _run(conv, bn, x, gup, False, **kw)
    _same(a, b)
    bn.load_state_dict(state)
    bn.eval()                                            # eval-mode BatchNorm: cb is whatever mrla_bn_stats_bwd wrote
    _same(_run(conv, bn, x, gup, True, **kw), _run(conv, bn, x, gup, False, **kw))


def test_deferred_form_returns_the_raw_output_and_the_affine():
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, _ = _inputs()
    out = Fm.conv_bn_act(x.clone().requires_grad_(True), conv, bn, relu=False, defer=True)
    assert "_ConvBnFn" in type(out.grad_fn).__name__
    assert out.shape == (2, 256, 8, 8) and out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
    assert (out.float().mean((0, 2, 3)).abs() > 1e-4).any()          # not normalised: the convolution's own output
    sc, sh = out._mrla_affine
    assert sc.shape == sh.shape == (256,) and not sc.requires_grad and out._mrla_bn_box is not None


def test_hook_second_consumer_and_autograd_grad_see_true_gradients():
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()
    c2 = torch.roll(gup, 1, 0)
    seen = {}

    def loss(out):
        out.register_hook(lambda gr: seen.setdefault("g", []).append(gr.detach().clone()))
        return (out * gup).sum() + (out.float() * c2.float()).sum()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, loss=loss, route="any")
    bn.load_state_dict(state)
    b = _run(conv, bn, x, gup, False, loss=loss)
    _same(a, b)
    assert len(seen["g"]) == 2 and torch.equal(seen["g"][0], seen["g"][1])
    # the layout of the summed gradient is autograd's choice: the route follows from what the hook saw arrive
    g0 = seen["g"][0]
    print("gradient at the node:", g0.dtype, tuple(g0.stride()))
    cl = g0.dtype == torch.bfloat16 and g0.is_contiguous(memory_format=torch.channels_last)
    _assert_route(a[5], "fused" if cl else "two_pass")
    assert torch.equal(seen["g"][0].float(), (gup.float() + c2.float()).bfloat16().float())
    xp = x.clone().requires_grad_(True)
    out = Fm.conv_bn_act(xp, conv, bn, relu=True)
    assert "_ConvBnFn" in type(out.grad_fn).__name__
    go, gx = torch.autograd.grad((out * gup).sum(), [out, xp])
    assert torch.equal(go, gup)
    assert torch.equal(gx, _run(conv, bn, x, gup, True)[0])


def test_frozen_weight_and_foreign_gradients_take_the_two_pass_route():
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    ref = _run(conv, bn, x, gup, False)
    # a gradient of another layout arrives at the one node: its backward runs the two passes, same values
    bn.load_state_dict(state)
    got = _run(conv, bn, x, gup.contiguous(), True, route="two_pass")
    _same(got, ref)
    conv.weight.requires_grad_(False)
    bn.load_state_dict(state)
    frozen = _run(conv, bn, x, gup, True, fused_expected=False, route="two_pass", wgrad=False)
    assert frozen[1] is None and torch.equal(frozen[0], ref[0]) and torch.equal(frozen[2], ref[2])


def test_a_shape_with_four_k_tiles_keeps_the_two_nodes():
    """k = 1024: mrla_conv1x1_wgrad_bn_supported says no (every k-tile would form dy again), so the pair stays two nodes."""
    from mrla_amd import _lib as L
    assert L.load().mrla_conv1x1_wgrad_bn_supported(128, 1024, 256, L.BF16) == L.EUNSUPPORTED
    conv, bn = _pair(k=1024, n=256)
    x, gup = _inputs(k=1024, n=256)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, fused_expected=False, route="two_pass")
    bn.load_state_dict(state)
    _same(a, _run(conv, bn, x, gup, False))


def test_whole_bottleneck_agrees_with_the_two_pass_route():
    """Two complete runs of one MRLA_Bottleneck, WGRAD_BN on and off, at the bounds tests/test_shortcut_addend_gpu.py uses
    for two runs of one block (MIOpen's 3x3 between conv1 and conv3 is not bit-stable)."""
    from mrla_amd import functional as Fm
    from tests.test_block_bf16_gpu import _ulps
    from tests.test_shortcut_addend_gpu import _block_case, _run_block
    blk, x, gup = _block_case((256, 128, 2, 56))
    res = {}
    for on in (True, False):
        old, Fm.WGRAD_BN = Fm.WGRAD_BN, on
        try:
            with _recorded() as calls:
                res[on] = _run_block(blk, x, gup, True)
        finally:
            Fm.WGRAD_BN = old
        # conv1, conv3 and the strided downsample: three pairs, all on one route (bn2, behind MIOpen's 3x3, keeps its
        # apply pass either way, so the apply entries say nothing here)
        names = [n for n, _ in calls]
        assert names.count("mrla_conv1x1_wgrad_bn") == (3 if on else 0), names
        assert names.count("mrla_conv1x1_wgrad") == (0 if on else 3), names
    (out1, dx1, gr1), (out0, dx0, gr0) = res[True], res[False]
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


def test_captured_forward_backward_replays_equal_eager():
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    want = _run(conv, bn, x, gup, True)
    xs = x.clone().requires_grad_(True)

    def step():
        out = Fm.conv_bn_act(xs, conv, bn, relu=True)
        assert "_ConvBnFn" in type(out.grad_fn).__name__
        out.backward(gup)
        return out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    conv.zero_grad(set_to_none=True)
    bn.zero_grad(set_to_none=True)
    bn.load_state_dict(state)
    graph = torch.cuda.CUDAGraph()
    with _recorded() as calls, torch.cuda.graph(graph):
        out = step()
    _assert_route(calls, "fused")
    for _ in range(2):
        bn.load_state_dict(state)
        graph.replay()
        torch.cuda.synchronize()
        got = (xs.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad, out.detach())
        for name, u, v in zip(("dx", "dW", "dgamma", "dbeta", "out"), got, want):
            assert torch.equal(u, v), f"{name}: {int((u != v).sum())} of {u.numel()} elements differ from the eager run"


def test_backward_leaves_no_reference_cycle_behind():
    """The deferred output and the passthrough output carry the node as their grad_fn; the backward must not park the
    unpacked saved tensors where the node keeps them alive (the whole graph in front of it would never be freed)."""
    import gc
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()

    def once():
        conv.zero_grad(set_to_none=True)
        bn.zero_grad(set_to_none=True)
        xp = (x.clone().requires_grad_(True) * 1.0)
        out, through = Fm.conv_bn_act(xp, conv, bn, relu=False, defer=True, passthrough=True)
        assert "_ConvBnFn" in type(out.grad_fn).__name__
        torch.autograd.backward([out, through], [gup, torch.ones_like(through)])
        conv.zero_grad(set_to_none=True)
        bn.zero_grad(set_to_none=True)
    with _recorded() as calls:
        once()
    _assert_route(calls, "fused")
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for _ in range(3):
        once()
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


# ------------------------------------------------------------------------------------------------------
# the fp16 rounding of the apply pass itself (as_f32_result, mrla_device.h)
# ------------------------------------------------------------------------------------------------------
def _apply_reference(g, xb, sc, sh, cb, relu):
    """fp16(fp32(e*dz + fp32(f*x + h))): the two fp32 fused multiply-adds through float64 (a product of two fp32 values is
    exact there; rounding the float64 sum to fp32 differs from one direct rounding about once in 2^29 elements), then what
    a torch cast of the fp32 value gives."""
    x64, g64 = xb.double(), g.double()
    z = (sc.double() * x64 + sh.double()).float()
    dz = torch.where(z > 0, g64, torch.zeros_like(g64)) if relu else g64
    t = (cb[:, 1].double() * x64 + cb[:, 2].double()).float()
    return (cb[:, 0].double() * dz + t.double()).float().half()


@pytest.mark.parametrize("c", [64, 96], ids=["flat", "strided"])
def test_fp16_apply_rounds_the_fp32_value_in_both_loops(c):
    """A behaviour change of mrla_bn_act_bwd for fp16 that came with the fused kernel: the fp32 result is rounded to fp16 as
    a torch cast rounds it, for every element.  Before, the unrolled main loop of the flat kernel did that and its tail loop
    rounded the exact fused multiply-add result once; the same element came out an fp16 ulp apart depending on the size of
    the tensor.  c = 64, m = 420 000: 13 125 iterations per thread column -> iters = 4, the main loop and the tail loop both
    run; the first 1000 rows alone run the tail loop only (iters = 1).  c = 96 is the strided kernel (not a power of two).
    One fp16 element in about 2^13 sits where the two roundings differ, so either size shows a change."""
    from mrla_amd import _lib as L
    gen = torch.Generator(device="cuda").manual_seed(90 + c)
    m = 420000 if c == 64 else 3000
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)       # noqa: E731
    g, xb = rnd(m, c).half(), rnd(m, c).half()
    sc, sh = torch.rand((c,), device="cuda", generator=gen) + 0.5, rnd(c) * 0.5
    cb = torch.stack([torch.rand((c,), device="cuda", generator=gen) + 0.5, rnd(c) * 0.25, rnd(c) * 0.1], dim=1).contiguous()

    def run(rows, relu):
        out = torch.full((rows, c), float("nan"), dtype=torch.float16, device="cuda")
        gs, xs = g[:rows].contiguous(), xb[:rows].contiguous()
        L.call("mrla_bn_act_bwd", _P(gs), _P(xs), _P(sc), _P(sh), _P(cb), relu, _P(out), 1, c, rows, 1, L.F16, L.NHWC, _stream())
        torch.cuda.synchronize()
        return out
    for relu in (0, 1):
        want = _apply_reference(g, xb, sc, sh, cb, relu)
        whole, head = run(m, relu), run(1000, relu)
        assert torch.equal(whole[:1000], head), f"{int((whole[:1000] != head).sum())} elements depend on the tensor's size"
        assert torch.equal(whole, want), f"{int((whole != want).sum())} of {want.numel()} elements differ from the cast"
