"""mrla_conv1x1_wgrad_bn_dx: the BN weight-gradient GEMM that also forms the convolution's input gradient dx = dy w for its own
pixel chunks and writes no dy (mrla_amd/csrc/conv1x1_wgrad.hip), and the branch of functional._ConvBnFn that takes it
(functional.WGRAD_BN_DX; reference call sites resnet_mrla_light.py:100-101, 196-199: stage 1's conv3 and downsample).

Kernel level, through the C ABI, k = 64, n = 256: the one launch against mrla_conv1x1_wgrad_bn followed by
mrla_conv1x1_fwd(dy_out, wt, ...) ON THE SAME INPUTS, bit for bit (torch.equal) on part, dw and dx.  Outputs are pre-filled
with NaN, dx carries 64 guard rows behind row m that must stay NaN.  Every case asserts the pipeline situation it is there
for from mrla_conv1x1_wgrad_plan (chunks per workgroup against the four LDS stages, both parities -- the two wave pairs
alternate chunks --, a short last range, a ragged last chunk).
Module level: conv_bn_act with functional.WGRAD_BN_DX on against off, torch.equal on dx, dW, dgamma, dbeta, and the C-ABI
entries the backward asked for."""
import gc

import pytest
import torch

from tests.test_conv1x1_wgrad_bn_gpu import _P, _TD, _inputs, _pair, _recorded, _situation, _stream

pytestmark = pytest.mark.gpu

K, N, GUARD = 64, 256, 64
DX_GEMMS = ("mrla_conv1x1_fwd", "mrla_conv1x1_fwd_add", "mrla_conv1x1_fwd_addend")

# m: (chunks per workgroup, the last workgroup's range ends short, the last chunk is ragged)
CASES = {1000: (1, False, True), 8192: (1, False, False), 16400: (3, False, True), 24600: (4, True, True),
         40960: (5, False, False), 50000: (7, True, True)}


def _kernel_case(m, dtype, relu, dw32, seed, again=False):
    from mrla_amd import _lib as L
    lib = L.load()
    td, dt = _TD[dtype], (L.BF16 if dtype == "bf16" else L.F16)
    assert lib.mrla_conv1x1_wgrad_bn_dx_supported(m, K, N, dt) == 1
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)       # noqa: E731
    g, xb, x = rnd(m, N).to(td), rnd(m, N).to(td), rnd(m, K).to(td)
    sc = torch.rand((N,), device="cuda", generator=gen) + 0.5
    sc[::7] = 0.0                                        # bn3's zero-initialised scale: z = sh, the mask is per channel
    sc[3::11] *= -1.0
    sh = rnd(N) * 0.5
    cb = torch.stack([torch.rand((N,), device="cuda", generator=gen) + 0.5, rnd(N) * 0.25,
                      rnd(N) * 0.1 + 300.0], dim=1).contiguous()      # a large h: a row past M that leaked would show
    w = (rnd(N, K) * 0.05).to(td)
    wt = w.t().contiguous()
    wdt, wtd = (L.F32, torch.float32) if dw32 else (dt, td)
    rows = lib.mrla_conv1x1_wgrad_rows(m, K, N, dt)
    assert rows == _situation(m, K, N, dt)[3]            # every row of part is written

    def bufs():
        return (torch.full((m + GUARD, K), float("nan"), dtype=td, device="cuda"),
                torch.full((rows, N, K), float("nan"), dtype=torch.float32, device="cuda"),
                torch.full((N, K), float("nan"), dtype=wtd, device="cuda"))
    dx0, part0, dw0 = bufs()
    dy0 = torch.full((m, N), float("nan"), dtype=td, device="cuda")
    L.call("mrla_conv1x1_wgrad_bn", _P(g), _P(xb), _P(sc), _P(sh), _P(cb), relu, _P(dy0), _P(x), _P(part0), _P(dw0),
           m, K, N, dt, wdt, _stream())
    L.call("mrla_conv1x1_fwd", _P(dy0), _P(wt), _P(dx0), None, m, N, K, dt, _stream())

    def fused():
        dx1, part1, dw1 = bufs()
        L.call("mrla_conv1x1_wgrad_bn_dx", _P(g), _P(xb), _P(sc), _P(sh), _P(cb), relu, _P(x), _P(wt), _P(dx1), _P(part1),
               _P(dw1), m, K, N, dt, wdt, _stream())
        torch.cuda.synchronize()
        return dx1, part1, dw1
    dx1, part1, dw1 = fused()
    assert torch.isfinite(dy0.float()).all() and dy0.float().abs().max() > 100          # h arrived
    assert torch.isfinite(dx0[:m].float()).all() and torch.isfinite(part0).all() and torch.isfinite(dw0.float()).all()
    assert dx0[:m].float().abs().max() > 1
    assert torch.isnan(dx0[m:].float()).all() and torch.isnan(dx1[m:].float()).all(), "a row at or past m was stored"
    ndx = int((dx1[:m] != dx0[:m]).sum())
    print(f"m={m} {dtype} relu={relu}: dx {ndx} of {m * K} elements differ, part {int((part1 != part0).sum())}, "
          f"dw {int((dw1 != dw0).sum())}")
    assert torch.equal(part1, part0), f"part: {int((part1 != part0).sum())} of {part0.numel()} elements differ"
    assert torch.equal(dw1, dw0), f"dw: {int((dw1 != dw0).sum())} of {dw0.numel()} elements differ"
    assert torch.equal(dx1[:m], dx0[:m]), f"dx: {ndx} of {m * K} elements differ"
    if again:
        dx2, part2, dw2 = fused()
        for u, v in ((dx2[:m], dx1[:m]), (part2, part1), (dw2, dw1)):
            assert torch.equal(u, v)


@pytest.mark.parametrize("relu", [0, 1], ids=["lin", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("m", sorted(CASES))
def test_one_launch_equals_the_two(m, dtype, relu):
    from mrla_amd import _lib as L
    cpw, short, ragged = CASES[m]
    plan = L.conv1x1_wgrad_plan(m, K, N, L.BF16)
    assert (plan[0], plan[1], plan[2], plan[3], plan[5]) == (cpw, 4, 256, 64, 1), plan
    assert _situation(m, K, N, L.BF16)[1] == short and (m % 32 != 0) == ragged
    # dw in the operands' type and in fp32, both under both relu settings across the cases; fp16 dw only where it cannot
    # overflow (thousands of pixels of |dy| ~ h = 300 sum past 65504)
    dw32 = 1 if (dtype == "f16" and m > 1000) else (relu ^ (sorted(CASES).index(m) & 1))
    _kernel_case(m, dtype, relu, dw32, seed=9000 + m + relu)


def test_the_cases_cover_the_pipeline_situations():
    cpws = [c[0] for c in CASES.values()]
    assert cpws.count(1) == 2 and {3, 4, 5, 7} <= set(cpws)                 # below, at and above the four stages; both parities
    assert any(c[1] for c in CASES.values()) and any(not c[2] for c in CASES.values())


def test_two_runs_give_the_same_bits():
    _kernel_case(24600, "bf16", 1, 1, seed=77, again=True)


# ------------------------------------------------------------------------------------------------------
# module level
# ------------------------------------------------------------------------------------------------------
def _run(conv, bn, x, gup, on, relu=True, defer=False, route=None, x_grad=True, ask=True):
    """One forward + backward of conv_bn_act(..., fuse_dx=ask), as the bottleneck calls it, with WGRAD_BN_DX = on: (dx, dW, dgamma, dbeta).  The entries the BACKWARD asked
    for are held to `route`: 'dx' (the one launch, no mrla_conv1x1_wgrad_bn, no input-gradient GEMM), 'two' (the reverse),
    'none' (neither form: the pair is not one node)."""
    from mrla_amd import functional as Fm
    old, Fm.WGRAD_BN_DX = Fm.WGRAD_BN_DX, on
    try:
        conv.zero_grad(set_to_none=True)
        bn.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(x_grad)
        out = Fm.conv_bn_act(xp, conv, bn, relu=relu, defer=defer, fuse_dx=ask)
        assert ("_ConvBnFn" in type(out.grad_fn).__name__) == (route != "none")
        with _recorded() as calls:
            out.backward(gup)
            torch.cuda.synchronize()
    finally:
        Fm.WGRAD_BN_DX = old
    _assert_route(calls, route or ("dx" if on else "two"), x_grad)
    return (xp.grad.clone() if x_grad else None, conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())


def _assert_route(calls, route, x_grad=True):
    names = [n for n, _ in calls]
    gemms = [n for n in names if n in DX_GEMMS]
    if route == "dx":
        assert names.count("mrla_conv1x1_wgrad_bn_dx") == 1 and "mrla_conv1x1_wgrad_bn" not in names and not gemms, names
    elif route == "two":
        assert names.count("mrla_conv1x1_wgrad_bn") == 1 and "mrla_conv1x1_wgrad_bn_dx" not in names, names
        assert len(gemms) == (1 if x_grad else 0), names
    else:
        assert "mrla_conv1x1_wgrad_bn_dx" not in names and "mrla_conv1x1_wgrad_bn" not in names, names


def _same(a, b):
    for name, u, v in zip(("dx", "dW", "dgamma", "dbeta"), a, b):
        assert torch.isfinite(u.float()).all(), name
        assert torch.equal(u, v), f"{name}: {int((u != v).sum())} of {u.numel()} elements differ"
    assert a[0].float().abs().max() > 0 and a[1].float().abs().max() > 0


def _ragged_inputs(seed=5):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((2, 64, 9, 7), device="cuda", generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    gup = torch.randn((2, 256, 9, 7), device="cuda", generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    return x, gup


@pytest.mark.parametrize("shape", ["8x8", "9x7"])
@pytest.mark.parametrize("form", ["relu", "linear", "deferred"])          # (a deferred BatchNorm cannot carry a ReLU)
def test_switch_on_equals_switch_off(form, shape):
    relu, defer = form == "relu", form == "deferred"
    conv, bn = _pair()
    x, gup = _inputs() if shape == "8x8" else _ragged_inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, relu=relu, defer=defer)
    bn.load_state_dict(state)
    b = _run(conv, bn, x, gup, False, relu=relu, defer=defer)
    _same(a, b)


def test_a_call_site_that_does_not_ask_keeps_the_two_launch_route():
    """conv_bn_act without fuse_dx launches what it always launched, whatever the switch says (the entry names of that route
    are what tests/test_conv1x1_wgrad_bn_gpu.py pins); the bottleneck's conv3 and downsample ask."""
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, route="two", ask=False)
    bn.load_state_dict(state)
    _same(a, _run(conv, bn, x, gup, True, route="dx"))


def test_stage_1_bottleneck_asks_for_conv3_and_the_downsample():
    """MRLA_Bottleneck(64 -> 64 -> 256, stride 1, with downsample) as the model runs it: two pairs on the one launch with the
    switch on, none with it off, and the block's results at the bounds tests/test_conv1x1_wgrad_bn_gpu.py uses for two runs
    of one block (MIOpen's 3x3 between conv1 and conv3 is not bit-stable)."""
    from mrla_amd import functional as Fm
    from tests.test_block_bf16_gpu import _ulps
    from tests.test_shortcut_addend_gpu import _block_case, _run_block
    blk, x, gup = _block_case((64, 64, 1, 56))
    res = {}
    for on in (True, False):
        old, Fm.WGRAD_BN_DX = Fm.WGRAD_BN_DX, on
        try:
            with _recorded() as calls:
                res[on] = _run_block(blk, x, gup, True)
        finally:
            Fm.WGRAD_BN_DX = old
        names = [n for n, _ in calls]
        assert names.count("mrla_conv1x1_wgrad_bn_dx") == (2 if on else 0), names
        assert names.count("mrla_conv1x1_wgrad_bn") == (1 if on else 3), names          # conv1 (shortcut addend) either way
    (out1, dx1, gr1), (out0, dx0, gr0) = res[True], res[False]
    assert torch.isfinite(dx1.float()).all() and dx1.float().abs().max() > 0
    assert (_ulps(out1, out0.double()) > 2.0).float().mean().item() < 1e-3
    assert (_ulps(dx1, dx0.double()) > 2.0).float().mean().item() < 5e-2
    assert gr1.keys() == gr0.keys()
    for name in gr1:
        den = gr0[name].float().norm().item()
        assert (gr1[name].float() - gr0[name].float()).norm().item() / max(den, 1e-30) < 1e-2, name


def test_frozen_input_keeps_the_two_launch_route():
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, route="two", x_grad=False)
    bn.load_state_dict(state)
    b = _run(conv, bn, x, gup, False, route="two", x_grad=False)
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)


def test_shortcut_gradient_arriving_keeps_the_two_launch_route():
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    res = {}
    for on in (True, False):
        old, Fm.WGRAD_BN_DX = Fm.WGRAD_BN_DX, on
        try:
            bn.load_state_dict(state)
            conv.zero_grad(set_to_none=True)
            bn.zero_grad(set_to_none=True)
            xp = x.clone().requires_grad_(True)
            out, through = Fm.conv_bn_act(xp, conv, bn, relu=False, defer=True, passthrough=True, fuse_dx=True)
            assert "_ConvBnFn" in type(out.grad_fn).__name__
            with _recorded() as calls:
                torch.autograd.backward([out, through], [gup, torch.ones_like(through)])
                torch.cuda.synchronize()
        finally:
            Fm.WGRAD_BN_DX = old
        _assert_route(calls, "two")
        res[on] = (xp.grad.clone(), conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())
    _same(res[True], res[False])


def test_fp16_pair_keeps_its_two_nodes():
    conv, bn = _pair()
    conv = conv.half()
    x, gup = _inputs()
    _run(conv, bn, x.half(), gup.half(), True, route="none")


def test_a_128_to_512_pair_keeps_the_two_launch_route():
    from mrla_amd import _lib as L
    assert L.load().mrla_conv1x1_wgrad_bn_dx_supported(128, 128, 512, L.BF16) == L.EUNSUPPORTED
    conv, bn = _pair(k=128, n=512)
    x, gup = _inputs(k=128, n=512)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    a = _run(conv, bn, x, gup, True, route="two")
    bn.load_state_dict(state)
    _same(a, _run(conv, bn, x, gup, False, route="two"))


def test_captured_forward_backward_replays_equal_eager():
    from mrla_amd import functional as Fm
    assert Fm.WGRAD_BN
    conv, bn = _pair()
    x, gup = _inputs()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    want = _run(conv, bn, x, gup, True)
    xs = x.clone().requires_grad_(True)
    old, Fm.WGRAD_BN_DX = Fm.WGRAD_BN_DX, True
    try:
        def step():
            out = Fm.conv_bn_act(xs, conv, bn, relu=True, fuse_dx=True)
            assert "_ConvBnFn" in type(out.grad_fn).__name__
            out.backward(gup)
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
            step()
        assert [n for n, _ in calls].count("mrla_conv1x1_wgrad_bn_dx") == 1
        assert not [n for n, _ in calls if n == "mrla_conv1x1_wgrad_bn"]
        for _ in range(2):
            bn.load_state_dict(state)
            graph.replay()
            torch.cuda.synchronize()
            got = (xs.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad)
            for name, u, v in zip(("dx", "dW", "dgamma", "dbeta"), got, want):
                assert torch.equal(u, v), f"{name}: {int((u != v).sum())} of {u.numel()} elements differ from the eager run"
    finally:
        Fm.WGRAD_BN_DX = old


def test_backward_leaves_no_reference_cycle_behind():
    """tests/test_conv1x1_wgrad_bn_gpu.py's allocator check on the new branch: the deferred output carries the node as its
    grad_fn, and the branch returns from inside the try whose finally clears the unpacked saved tensors."""
    from mrla_amd import functional as Fm
    conv, bn = _pair()
    x, gup = _inputs()
    old, Fm.WGRAD_BN_DX = Fm.WGRAD_BN_DX, True
    try:
        def once():
            conv.zero_grad(set_to_none=True)
            bn.zero_grad(set_to_none=True)
            xp = (x.clone().requires_grad_(True) * 1.0)
            out = Fm.conv_bn_act(xp, conv, bn, relu=False, defer=True, fuse_dx=True)
            assert "_ConvBnFn" in type(out.grad_fn).__name__
            out.backward(gup)
            conv.zero_grad(set_to_none=True)
            bn.zero_grad(set_to_none=True)
        with _recorded() as calls:
            once()
        assert "mrla_conv1x1_wgrad_bn_dx" in [n for n, _ in calls]
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(3):
            once()
        gc.collect()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == base
    finally:
        Fm.WGRAD_BN_DX = old
