"""GPU, route level: the stride-1 3x3 input gradient as the stock forward convolution on banked flipped weights
(functional.CONV3X3_DGRAD_FLIP, Conv3x3Bank, mrla_conv3x3_dgrad_flip_preferred, mrla_conv3x3_weight_bank_refresh).

The shapes come from the rule itself: per channel width of ResNet-50 on its map, the smallest batch it answers 1 for.
  * the rule at its edge: 1 there, 0 one image below, 0 at the small shapes of tests/launch_trace_cases.py;
  * at each of those shapes, bf16: x.grad of the routed call inside |dx - dx64| <= u |dx64| + (1 + u) 9 n 2^-24 A of the float64
    gradient from the same rounded operands (A: that gradient of |dy|, |w|; the bound of tests/test_conv3x3_fwd_gpu.py for its
    dx) and within 2 ulps (at the tensor's largest magnitude) of the unrouted call under cudnn.deterministic; the output and
    weight.grad bit-equal to the unrouted call's;
  * integer-valued data whose sums are exact in fp32 and in bf16: the routed dx IS the float64 one;
  * one +inf in dy: dx is non-finite only where the stock gradient is;
  * a routed block step refreshes the bank exactly once per forward and runs no per-call permutation or weight cast; a model
    whose shapes all answer 0 never calls the entry point; graphed_step on routed blocks checks out (verify=3) and a first use
    inside a capture raises MrlaHipError; with the switch off graph, launches and values are those of a call without a bank."""
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
WIDTHS = [(64, 56), (128, 28), (256, 14), (512, 7)]          # (channels, map) of the stride-1 3x3 convolutions of ResNet-50
U = 2.0 ** -8                                                # unit roundoff of bf16


def _rule(b, c, h, w, dt=None):
    from mrla_amd import _lib as L
    return L.load().mrla_conv3x3_dgrad_flip_preferred(b, c, c, h, w, L.BF16 if dt is None else dt)


@functools.lru_cache(None)
def _smallest_batch(c, hw):
    for b in range(1, 4097):
        if _rule(b, c, hw, hw) == 1:
            return b
    raise AssertionError(f"the rule routes no batch up to 4096 at {c} channels on {hw} x {hw}")


@contextlib.contextmanager
def _deterministic():
    was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        yield
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = was


@contextlib.contextmanager
def _recorded_calls():
    """The names of the C-ABI entry points called inside, in order."""
    from mrla_amd import _lib as L
    names, orig = [], L.call
    L.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
    try:
        yield names
    finally:
        L.call = orig


def _conv(c, w=None):
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=False).cuda().to(memory_format=CL)
    if w is not None:
        with torch.no_grad():
            conv.weight.copy_(w)
    return conv


def _call(conv, x, dy, routed, bank=None):
    """One forward and backward of F.conv3x3 under bf16 autocast: (out, dx, dw, grad_fn type name, entry points called).
    routed: inside a bookkeeping scope with a Conv3x3Bank; else with the switch off and no scope."""
    from mrla_amd import functional as F
    conv.weight.grad = None
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    scope = F.batched_bookkeeping(0, None, bank if bank is not None else F.Conv3x3Bank()) if routed else F.conv3x3_dgrad_flip(False)
    with _recorded_calls() as names, scope, torch.autocast("cuda", dtype=torch.bfloat16):
        out = F.conv3x3(x, conv)
        node = type(out.grad_fn).__name__
        out.backward(dy)
    torch.cuda.synchronize()
    return out.detach(), x.grad, conv.weight.grad, node, list(names)


def _dx64(dy, w, shape):
    """The float64 input gradient on the CPU, by autograd."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, w, padding=1).backward(dy)
    return x.grad


@functools.lru_cache(None)
def _case(c, hw):
    """Operands at the smallest routed batch of a width, the routed and the unrouted call, and the float64 reference."""
    from mrla_amd import functional as F
    b = _smallest_batch(c, hw)
    g = torch.Generator(device="cuda").manual_seed(c)
    x = torch.randn((b, c, hw, hw), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL)
    dy = torch.randn((b, c, hw, hw), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL)
    conv = _conv(c)
    with _deterministic(), F.conv3x3_dgrad_flip(True):
        routed = _call(conv, x, dy, True)
        stock = _call(conv, x, dy, False)
    w16 = conv.weight.detach().bfloat16()
    dy64, w64 = dy.double().cpu(), w16.double().cpu()
    shape = tuple(x.shape)
    return dict(b=b, x=x, dy=dy, conv=conv, routed=routed, stock=stock, dx64=_dx64(dy64, w64, shape),
                a=_dx64(dy64.abs(), w64.abs(), shape))


def test_the_rule_at_its_edge():
    from mrla_amd import _lib as L
    for c, hw in WIDTHS:
        b = _smallest_batch(c, hw)
        assert b > 1 and _rule(b, c, hw, hw) == 1 and _rule(b - 1, c, hw, hw) == 0, (c, hw, b)
        print(f"{c} channels on {hw} x {hw}: routed from batch {b}")
    assert _rule(2, 64, 16, 16) == 0 and _rule(8, 64, 16, 16) == 0
    # stride 2 has no such route: the rule is asked for stride 1 only, and conv3x3 never asks it for a strided convolution
    from mrla_amd import functional as F
    for c, hw in WIDTHS[:2]:
        conv = torch.nn.Conv2d(c, c, 3, stride=2, padding=1, bias=False).cuda().to(memory_format=CL)
        b = _smallest_batch(c, hw)
        x = torch.randn((b, c, hw, hw), device="cuda").bfloat16().contiguous(memory_format=CL).requires_grad_(True)
        bank = F.Conv3x3Bank()
        assert F.Conv3x3Bank.eligible(conv) is False
        with F.conv3x3_dgrad_flip(True), F.batched_bookkeeping(0, None, bank), torch.autocast("cuda", dtype=torch.bfloat16):
            assert F._conv3x3_banked(conv, x, True) is None
        assert bank.members == []
    assert _rule(256, 64, 56, 56, L.F16) == 0


@pytest.mark.parametrize("c,hw", WIDTHS, ids=lambda v: str(v))
def test_the_routed_gradient_at_the_smallest_routed_batch(c, hw):
    case = _case(c, hw)
    out, dx, dw, node, names = case["routed"]
    out0, dx0, dw0, node0, names0 = case["stock"]
    assert node == "_Conv3x3FnBackward" and names.count("mrla_conv3x3_weight_bank_refresh") == 1
    assert "mrla_conv3x3_weight_bank_refresh" not in names0
    assert dx.dtype == torch.bfloat16 and dx.shape == case["x"].shape and dx.is_contiguous(memory_format=CL)
    want64, a = case["dx64"], case["a"]
    err = (dx.double().cpu() - want64).abs()
    excess = float((err - U * want64.abs()).clamp_min(0).div(a.clamp_min(1e-300)).max())
    top = float(dx0.abs().max())
    ulp = 2.0 ** (torch.tensor(top).log2().floor().item() - 7)
    apart = float((dx.double() - dx0.double()).abs().max())
    print(f"b{case['b']} {c}->{c} {hw}x{hw}: max (|dx - dx64| - u |dx64|)+ / A = {excess:.3e} (fp32 term of the bound "
          f"{9 * c * 2.0 ** -24:.3e}); routed against unrouted: max |diff| = {apart:.3e} = {apart / ulp:.2f} ulps at max |dx| = "
          f"{top:.3e}, {int((dx != dx0).sum())} of {dx.numel()} elements differ")
    bound = U * want64.abs() + (1 + U) * 9 * c * 2.0 ** -24 * a
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"
    assert apart <= 2 * ulp, (apart, ulp)
    assert torch.equal(out.view(torch.int16), out0.view(torch.int16))
    assert dw.dtype == dw0.dtype and dw.stride() == dw0.stride() == case["conv"].weight.stride()
    assert torch.equal(dw, dw0)


def test_integer_valued_data_gives_the_float64_gradient_bit_for_bit():
    from mrla_amd import functional as F
    c, hw = WIDTHS[0]
    b = _smallest_batch(c, hw)
    g = torch.Generator(device="cuda").manual_seed(11)
    # |dy| <= 1 and |w| <= 1 with 16 output channels in use: at most 144 terms of magnitude 1 -- every sum an integer below 256,
    # exact in fp32 in any order and exact in bf16
    dy = torch.randint(-1, 2, (b, c, hw, hw), device="cuda", generator=g).bfloat16().contiguous(memory_format=CL)
    w = torch.randint(-1, 2, (c, c, 3, 3), device="cuda", generator=g).float()
    w[16:] = 0
    x = torch.zeros((b, c, hw, hw), device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
    conv = _conv(c, w)
    with F.conv3x3_dgrad_flip(True):
        _, dx, _, node, names = _call(conv, x, dy, True)
    assert node == "_Conv3x3FnBackward" and names.count("mrla_conv3x3_weight_bank_refresh") == 1
    want64 = _dx64(dy.double().cpu(), w.double().cpu(), tuple(x.shape))
    assert float(want64.abs().max()) >= 8 and float(want64.abs().max()) <= 144
    assert torch.equal(dx.double().cpu(), want64)


def test_an_infinite_gradient_element_spreads_only_where_the_stock_gradient_is_non_finite():
    from mrla_amd import functional as F
    c, hw = WIDTHS[3]
    case = _case(c, hw)
    dy = case["dy"].clone(memory_format=torch.preserve_format)
    n0 = 37
    dy[1, n0, 3, 4] = float("inf")
    with _deterministic(), F.conv3x3_dgrad_flip(True):
        _, dx, _, _, names = _call(case["conv"], case["x"], dy, True)
        _, dx0, _, _, _ = _call(case["conv"], case["x"], dy, False)
    assert names.count("mrla_conv3x3_weight_bank_refresh") == 1
    bad, bad0 = ~torch.isfinite(dx), ~torch.isfinite(dx0)
    assert bool(bad0.any()) and bool(bad.any())
    assert not bool((bad & ~bad0).any())                              # only where the stock gradient is non-finite
    assert not bool(bad[0].any()) and not bool(bad[2:].any())         # one image, and there the 3 x 3 window of the element
    window = torch.zeros_like(bad)
    window[1, :, 2:5, 3:6] = True
    assert not bool((bad & ~window).any())


class _Stack(torch.nn.Module):
    """Bottleneck blocks under one bookkeeping scope with a Conv3x3Bank, as a network's forward_features runs them."""

    def __init__(self, n_blocks=2):
        super().__init__()
        from mrla_amd import functional as F, resnet
        torch.manual_seed(0)
        self.blocks = torch.nn.Sequential(*[resnet.MRLA_Bottleneck(256, 64) for _ in range(n_blocks)])
        self.bank = F.Conv3x3Bank()
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                    m.weight.fill_(0.5)

    def forward(self, x):
        from mrla_amd import functional as F
        with F.batched_bookkeeping(0, None, self.bank):
            return self.blocks(x)


def _stack_and_input():
    c, hw = WIDTHS[0]
    b = _smallest_batch(c, hw)
    net = _Stack().cuda().to(memory_format=CL).train()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.relu(torch.randn((b, 256, hw, hw), device="cuda", generator=g)).bfloat16().contiguous(memory_format=CL)
    return net, x


def _op_shapes(prof, names):
    return [tuple(map(tuple, e.input_shapes[:1])) for e in prof.events() if e.name in names]


def test_a_routed_block_step_refreshes_once_per_forward_and_runs_no_per_call_permutation_or_cast():
    from mrla_amd import functional as F
    net, x = _stack_and_input()
    weights = [((64, 64, 3, 3),), ]

    def step(profile):
        ctx = (torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) if profile
               else contextlib.nullcontext())
        for p in net.parameters():
            p.grad = None
        with _recorded_calls() as names, ctx as prof, torch.autocast("cuda", dtype=torch.bfloat16):
            net(x).float().mean().backward()
        torch.cuda.synchronize()
        return list(names), prof

    with F.conv3x3_dgrad_flip(True):
        step(False)                                                  # the first forward builds the bank (once per new member)
        assert len(net.bank.members) == 2 and net.bank.members[0] is net.blocks[0].conv2
        for _ in range(2):
            names, prof = step(True)
            assert names.count("mrla_conv3x3_weight_bank_refresh") == 1, names
            # no flip anywhere, and no cast or copy of a 3x3 weight: the autocast cast of the master and the permuting copies
            assert _op_shapes(prof, ("aten::flip",)) == []
            moved = [s for s in _op_shapes(prof, ("aten::_to_copy", "aten::copy_", "aten::clone", "aten::contiguous")) if s in weights]
            assert moved == [], moved
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with F.conv3x3_dgrad_flip(False):                                # the same count on the unrouted step: the casts are there
        names, prof = step(True)
        assert "mrla_conv3x3_weight_bank_refresh" not in names
        moved = [s for s in _op_shapes(prof, ("aten::_to_copy",)) if s in weights]
        assert len(moved) >= 2, moved


def test_a_model_whose_shapes_all_answer_0_never_calls_the_entry_point():
    from mrla_amd import functional as F, resnet
    torch.manual_seed(0)
    net = resnet.resnet50_mrlal(num_classes=10).cuda().train()
    x = torch.randn(2, 3, 64, 64, device="cuda")
    with F.conv3x3_dgrad_flip(True), _recorded_calls() as names:
        for _ in range(2):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                net(x).float().mean().backward()
    torch.cuda.synchronize()
    assert "mrla_weight_bank_refresh_dt" in names and "mrla_conv3x3_weight_bank_refresh" not in names
    bank = net._conv3x3_bank()
    assert bank.members == [] and bank.entries == {} and bank.table is None


def test_a_captured_step_on_routed_blocks_checks_out_and_a_first_use_inside_a_capture_raises():
    import mrla_amd
    from mrla_amd import _lib as L, functional as F
    net, x = _stack_and_input()
    proj = torch.rand((x.shape[0], 256, x.shape[2], x.shape[3]), device="cuda").contiguous(memory_format=CL)
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)
    with F.conv3x3_dgrad_flip(True):
        step = mrla_amd.graphed_step(net, opt, lambda out, p: (out * p).mean(), (x, proj), verify=3)
        print({k: step.report[k] for k in ("ok", "weights_rel_l2", "update_rel_l2", "noise_update_rel_l2")})
        assert step.report["ok"] is True and step.graph is not None
        assert len(net.bank.members) == 2 and net.bank.captured is True
        with _recorded_calls() as names:
            step(x, proj)
        assert step.last_launch == "graph" and names == []
        torch.cuda.synchronize()
        # a bank that has never run eagerly: its first use inside a capture is refused with a clear error
        conv = _conv(64)
        xs = x[:, :64].contiguous(memory_format=CL).requires_grad_(True)
        bank = F.Conv3x3Bank()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                with F.batched_bookkeeping(0, None, bank), torch.autocast("cuda", dtype=torch.bfloat16):
                    with pytest.raises(L.MrlaHipError, match="eagerly before capturing"):
                        F.conv3x3(xs, conv)
        except RuntimeError:
            pass                                                      # (an empty capture may itself be refused by the runtime)
        assert bank.members == [] and bank.entries == {}


def test_with_the_switch_off_graph_launches_and_values_are_those_of_a_call_without_a_bank():
    from mrla_amd import functional as F
    c, hw = WIDTHS[1]
    case = _case(c, hw)
    conv, x, dy = case["conv"], case["x"], case["dy"]
    bank = F.Conv3x3Bank()
    with _deterministic():
        with F.conv3x3_dgrad_flip(False):
            inside = _call(conv, x, dy, True, bank)                    # a bank in scope, the switch off
        plain = case["stock"]                                          # no scope at all: what a call always was
    assert bank.members == [] and bank.table is None
    assert inside[3] == plain[3] and inside[4] == plain[4] and "mrla_conv3x3_weight_bank_refresh" not in inside[4]
    for got, want in zip(inside[:3], plain[:3]):
        assert got.dtype == want.dtype and got.stride() == want.stride() and torch.equal(got, want)
