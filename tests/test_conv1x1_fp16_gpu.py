"""GPU parity of the fp16 forms of the 1x1-convolution GEMMs (mrla_conv1x1_* with MRLA_F16; resnet_mrla_light.py:93-102
conv1 / bn1, conv3 / bn3 and their backward), the fp16 weight bank and the fp16 autocast / model.half() routes through them.

Reference: a float64 product of the same fp16-rounded operands.  An fp16 output may differ from the once-rounded reference
by one fp16 ulp of the value (2^-10 relative) plus a floor: the larger of 1e-3 of the tensor's largest ulp (the bf16
helper's form) and 4 * E32, E32 being the largest deviation of a float32 numpy product of the same operands from the
float64 one -- what any fp32 accumulation of these terms does; the factor 4 covers the MFMA's different summation order.
Moment records are held to the bf16 tests' bound (1e-5 against float64 sums of the STORED outputs, every pixel counted
once).  The addend forms, the fp32 weight gradient, the weight bank and graph replays are compared bit for bit with the
paths they replace."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import detgen
from tests.test_light_gpu import relmax

pytestmark = pytest.mark.gpu

F16 = torch.float16
CL = torch.channels_last


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def f16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(F16).float().numpy()


def _operands(b, h, w, k, n, salt=0):
    """Seeded like tests/test_conv1x1_gpu.py, rounded to fp16.  Beyond 8209 pixels the rows repeat with that (prime) period,
    in step with no tile: the generator costs more than the kernels there."""
    s = detgen.seed_of(f"conv1x1/{b}/{h}/{k}/{n}/{salt}")
    m = b * h * w
    if m > 8209:
        x = f16_round(detgen.normalish((8209, k), s))[np.arange(m) % 8209].reshape(b, h, w, k)
    else:
        x = f16_round(detgen.normalish((b, h, w, k), s))
    wt = f16_round(detgen.normalish((n, k), s + 1) * (2.0 / k) ** 0.5)
    return x, wt


def _product(a, bt):
    """(float64 a @ bt.T, E32) for float32 numpy operands holding fp16 values: the reference and the deviation of a float32
    product of the same operands from it.  The float64 product runs on the GPU (these are up to 24 GFLOP)."""
    want = (torch.from_numpy(a).cuda().double() @ torch.from_numpy(bt).cuda().double().t()).cpu().numpy()
    e32 = float(np.abs((a @ bt.T).astype(np.float64) - want).max())
    return want, e32


def assert_f16_close(got, want64, e32, what):
    want = f16_round(want64)
    floor = max(1e-3 * np.abs(want64).max() * 2.0 ** -10, 4.0 * e32)
    err = np.abs(got - want)
    bad = err > np.abs(want64) * 2.0 ** -10 + floor
    print(f"{what}: worst |got - f16(want)| {err.max():.3e}, floor {floor:.3e} (E32 {e32:.3e}), max |want| {np.abs(want64).max():.3e}")
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} beyond 1 fp16 ulp + floor; worst {err.max()}"


def _check_records(part, got, m):
    from tests.test_conv1x1_gpu import raw_sums
    g64 = got.astype(np.float64)
    s = raw_sums(part).cpu().numpy()
    assert part[:, :, 3].double().sum(0).eq(m).all()             # every pixel counted once per channel
    r1, r2 = relmax(s[:, 0], g64.sum(0)), relmax(s[:, 1], (g64 * g64).sum(0))
    print(f"moment records: relmax sum {r1:.3e}, sum of squares {r2:.3e}")
    assert r1 < 1e-5 and r2 < 1e-5


# ---- 1. forward + records through _Conv1x1Fn ---------------------------------------------------------------------------
def _tile_m1(n):
    return 64 if n % 256 == 0 else 128            # pixel tile of the K-streaming kernel with one 32-pixel block per wave


def _smallest_m_with_two_blocks(k, n):
    """Smallest m for which ks_plan gives a wave two pixel blocks (pb = 2), read off the planner: one record row per pixel
    tile, and the tile doubles."""
    from mrla_amd import _lib as L
    lib, t1 = L.load(), _tile_m1(n)
    for m in range(2 * t1 + 1, 1 << 20):
        rows = lib.mrla_conv1x1_rows(m, k, n, L.F16)
        if rows == -(-m // (2 * t1)) and rows != -(-m // t1):
            assert lib.mrla_conv1x1_rows(m - 1, k, n, L.F16) == -(-(m - 1) // t1)      # one pixel fewer: still the small tile
            assert L.conv1x1_plan(m, k, n, dtype=L.F16)[1] == 3
            return m
    raise AssertionError("no pixel count with pb = 2")


def _smallest_m_with_the_big_tile(k, n):
    """Smallest m for which ks_plan takes the 256 x 256 tile (four LDS stages in mrla_conv1x1_plan's answer)."""
    from mrla_amd import _lib as L
    for m in range(1, 1 << 20, 256):              # (the choice depends on ceil(m / 256) only)
        if L.conv1x1_plan(m, k, n, dtype=L.F16)[1] == 4:
            assert L.conv1x1_plan(m - 1, k, n, dtype=L.F16)[1] == 3
            assert L.load().mrla_conv1x1_rows(m, k, n, L.F16) == -(-m // 256)
            return m
    raise AssertionError("no pixel count with the 256 x 256 tile")


FWD = [(1, 4, 8, 64, 64), (1, 1, 1, 256, 64), (3, 7, 7, 64, 128), (5, 12, 16, 128, 192),                   # narrow
       (1, 5, 7, 64, 256), (2, 9, 9, 128, 256), (1, 1, 1, 256, 256),                                      # wide
       (2, 7, 7, 512, 128), (2, 7, 7, 512, 256), (3, 5, 7, 544, 128),                                     # K-streaming
       ("pb2", 512, 1024), ("big", 1024, 256)]


@pytest.mark.parametrize("shape", FWD, ids=lambda s: "x".join(map(str, s)))
def test_forward_gemm_and_moment_records(shape):
    from mrla_amd import _lib as L, functional as Fm
    if shape[0] == "pb2":
        k, n = shape[1:]
        b, h, w = 1, 1, _smallest_m_with_two_blocks(k, n)
    elif shape[0] == "big":
        k, n = shape[1:]
        b, h, w = 1, 1, _smallest_m_with_the_big_tile(k, n)
    else:
        b, h, w, k, n = shape
    m = b * h * w
    if isinstance(shape[0], str):
        assert m % 32 != 0, m
    rows = L.load().mrla_conv1x1_rows(m, k, n, L.F16)
    assert rows > 0 and rows == L.load().mrla_conv1x1_rows(m, k, n, L.BF16)
    x, wt = _operands(b, h, w, k, n)
    xt = torch.from_numpy(x).cuda().half().permute(0, 3, 1, 2)                # [b, k, h, w], channels_last memory
    assert xt.is_contiguous(memory_format=CL)
    wtt = torch.from_numpy(wt).cuda().half()
    y, part = Fm._Conv1x1Fn.apply(xt, wtt, True)
    y2, p2 = Fm._Conv1x1Fn.apply(xt, wtt, False)
    torch.cuda.synchronize()
    assert y.dtype == F16 and y.is_contiguous(memory_format=CL) and tuple(part.shape) == (rows, n, L.GEMM_MOMENTS)
    assert p2.numel() == 0 and torch.equal(y, y2)                             # no records requested: same outputs
    want, e32 = _product(x.reshape(m, k), wt)
    got = y.permute(0, 2, 3, 1).reshape(m, n).float().cpu().numpy()
    assert_f16_close(got, want, e32, "y")
    _check_records(part, got, m)


# ---- 2. steady state ------------------------------------------------------------------------------------------------------
def _smallest_ragged_m(k, n):
    """The smallest ragged m (more than one 32-pixel block, the last one partial) the planner takes with >= 2 pipeline
    depths of units per workgroup (as tests/test_conv1x1_steady_gpu.py::_ragged_m, searched upwards)."""
    from mrla_amd import _lib as L
    plan, out = L.load().mrla_conv1x1_plan, (ctypes.c_int * 4)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for m in range(33, 1 << 20):
        if m % 32 and plan(m, k, n, L.F16, 0, ptr) == L.OK and out[0] >= 2 * out[1]:
            return m
    raise AssertionError("no ragged pixel count with a deep pipeline")


@pytest.mark.parametrize("shape", [(64, 64), (256, 256), (512, 128)], ids=["narrow", "wide", "kstream"])
def test_forward_gemm_in_steady_state(shape):
    from mrla_amd import _lib as L
    k, n = shape
    m = _smallest_ragged_m(k, n)
    upw, depth, _, rows = L.conv1x1_plan(m, k, n, dtype=L.F16)
    assert m % 32 and upw >= 2 * depth, (m, upw, depth)
    assert rows == L.load().mrla_conv1x1_rows(m, k, n, L.F16)
    x, wt = _operands(1, 1, m, k, n, salt=20)
    xt, wtt = torch.from_numpy(x).cuda().half().reshape(m, k), torch.from_numpy(wt).cuda().half()

    def run():
        y = torch.full((m, n), float("nan"), dtype=F16, device="cuda")
        part = torch.full((rows, n, L.GEMM_MOMENTS), float("nan"), dtype=torch.float32, device="cuda")
        L.call("mrla_conv1x1_fwd", _P(xt), _P(wtt), _P(y), _P(part), m, k, n, L.F16, _stream())
        return y, part
    (y, part), (y2, part2) = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs of the same launch differ"
    want, e32 = _product(x.reshape(m, k), wt)
    got = y.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert_f16_close(got, want, e32, "y")
    _check_records(part, got, m)


# ---- 3. addend forms ------------------------------------------------------------------------------------------------------
def _scatter(addc, b, h, w, n, sh, sw):
    full = torch.zeros((b, h, w, n), dtype=addc.dtype, device=addc.device)
    full[:, ::sh, ::sw] = addc
    return full.reshape(b * h * w, n)


ADDEND = [(3, 7, 7, 128, 64, "narrow"), (2, 5, 9, 64, 192, "narrow"), (3, 7, 7, 64, 256, "wide"), (2, 5, 9, 256, 512, "wide"),
          (3, 7, 7, 512, 128, "kstream"), (2, 5, 9, 1024, 256, "kstream")]


@pytest.mark.parametrize("stride", [1, 2], ids=["dense", "compact"])
@pytest.mark.parametrize("case", ADDEND, ids=lambda c: "x".join(map(str, c)))
def test_addend_forms_equal_the_paths_they_replace(case, stride):
    from mrla_amd import _lib as L
    lib = L.load()
    b, h, w, k, n, form = case
    m, sh, sw = b * h * w, stride, stride
    hc, wc = (h + sh - 1) // sh, (w + sw - 1) // sw
    wide = lib.mrla_conv1x1_add_supported(m, k, n, L.F16) == 1
    assert wide == (form == "wide") and (k >= 512) == (form == "kstream")
    assert lib.mrla_conv1x1_addend_supported(m, k, n, sh, sw, L.F16) == 1
    x, wt = _operands(b, h, w, k, n, salt=30)
    add = f16_round(detgen.normalish((b, hc, wc, n), detgen.seed_of(f"conv1x1/f16/add/{m}/{k}/{n}/{stride}")))
    xt, wtt = torch.from_numpy(x).cuda().half().reshape(m, k), torch.from_numpy(wt).cuda().half()
    addc = torch.from_numpy(add).cuda().half()
    full = _scatter(addc, b, h, w, n, sh, sw)
    nan = lambda: torch.full((m, n), float("nan"), dtype=F16, device="cuda")  # noqa: E731

    def run(dst, addend):
        L.call("mrla_conv1x1_fwd_addend", _P(xt), _P(wtt), _P(addend), _P(dst), m, k, n, b, h, w, sh, sw, L.F16, _stream())
        return dst
    y, y2 = run(nan(), addc), run(nan(), addc)
    ref = nan()
    if wide:          # fp32 sum, one rounding: the dense form on the scattered addend
        L.call("mrla_conv1x1_fwd_add", _P(xt), _P(wtt), _P(full), _P(ref), m, k, n, L.F16, _stream())
    else:             # f16(f16(x w^T) + addend): the GEMM followed by torch's fp16 add
        L.call("mrla_conv1x1_fwd", _P(xt), _P(wtt), _P(ref), None, m, k, n, L.F16, _stream())
        ref = ref + full
    torch.cuda.synchronize()
    assert torch.equal(y, y2), "two runs of the same launch differ"
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, ref), f"{int((y != ref).sum())} of {y.numel()} elements differ from the path it replaces"
    if stride == 1:
        inplace = addc.reshape(m, n).clone()
        run(inplace, inplace)
        torch.cuda.synchronize()
        assert torch.equal(inplace, y), "in place (addend aliasing y) differs"
        if wide:
            inplace = addc.reshape(m, n).clone()
            L.call("mrla_conv1x1_fwd_add", _P(xt), _P(wtt), _P(inplace), _P(inplace), m, k, n, L.F16, _stream())
            torch.cuda.synchronize()
            assert torch.equal(inplace, y)
    if wide:
        want, e32 = _product(x.reshape(m, k), wt)
        want = want + full.double().cpu().numpy()
        assert_f16_close(y.float().cpu().numpy(), want, e32, "y")


# ---- 4. weight gradient ---------------------------------------------------------------------------------------------------
def _wgrad_cases():
    from tests.test_conv1x1_gpu import WGRAD_SHAPES
    return sorted({(h, w, k, n) for _, h, w, k, n in WGRAD_SHAPES})


@pytest.mark.parametrize("shape", _wgrad_cases(), ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_gemm(shape):
    from mrla_amd import _lib as L
    lib = L.load()
    h, w, k, n = shape
    b = next(b for b in range(1, 200) if lib.mrla_conv1x1_wgrad_rows(b * h * w, k, n, L.F16) >= 2)   # the smallest batch with two splits
    m = b * h * w
    rows = lib.mrla_conv1x1_wgrad_rows(m, k, n, L.F16)
    assert rows >= 2 and rows == lib.mrla_conv1x1_wgrad_rows(m, k, n, L.BF16)
    x, _ = _operands(b, h, w, k, n, salt=3)
    dy = f16_round(detgen.normalish((b, h, w, n), detgen.seed_of(f"conv1x1/wgrad/dy/{m}/{k}/{n}")))
    xt, dyt = torch.from_numpy(x).cuda().half().reshape(m, k), torch.from_numpy(dy).cuda().half().reshape(m, n)

    def run(dtype, code):
        part = torch.full((rows, n, k), float("nan"), dtype=torch.float32, device="cuda")
        dw = torch.full((n, k), float("nan"), dtype=dtype, device="cuda")
        L.call("mrla_conv1x1_wgrad", _P(dyt), _P(xt), _P(part), _P(dw), m, k, n, L.F16, code, _stream())
        return part, dw
    (part, d16), (_, d32) = run(F16, L.F16), run(torch.float32, L.F32)
    torch.cuda.synchronize()
    want, e32 = _product(np.ascontiguousarray(dy.reshape(m, n).T), np.ascontiguousarray(x.reshape(m, k).T))   # the m-long sums
    got = d16.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert_f16_close(got, want, e32, "dw")
    r = relmax(part.double().sum(0).cpu().numpy(), want)
    print(f"partial tiles: relmax {r:.3e}")
    assert r < 1e-5
    assert torch.equal(d32.half(), d16)


# ---- 5. overflow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(75, 64, 64), (75, 64, 256)], ids=["narrow", "wide"])
def test_outputs_beyond_the_fp16_range_become_infinities(shape):
    """x = +-16 per pixel, w = +-128 on every third channel and +-16 on the others, k = 64: the outputs are exactly
    +-131072 (twice the largest fp16 and beyond: +-inf) or +-16384 (a quarter of it: stored exactly)."""
    from mrla_amd import _lib as L
    m, k, n = shape
    sx = torch.where(torch.arange(m) % 3 == 1, -16.0, 16.0)
    big = torch.arange(n) % 3 == 0
    sw = torch.where(torch.arange(n) % 5 < 2, -1.0, 1.0) * torch.where(big, 128.0, 16.0)
    x = sx[:, None].expand(m, k).contiguous().cuda().half()
    wt = sw[:, None].expand(n, k).contiguous().cuda().half()
    want = (x.double() @ wt.double().t())
    assert (want[:, big.cuda()].abs() >= 2 * 65504).all() and (want[:, ~big.cuda()].abs() <= 65504 / 2).all()
    y = torch.full((m, n), float("nan"), dtype=F16, device="cuda")
    L.call("mrla_conv1x1_fwd", _P(x), _P(wt), _P(y), None, m, k, n, L.F16, _stream())
    torch.cuda.synchronize()
    got = y.double()
    inf = torch.isinf(got)
    assert torch.equal(inf, want.abs() >= 2 * 65504)                       # infinities exactly there ...
    assert torch.equal(torch.sign(got), torch.sign(want))                  # ... with the product's sign
    assert torch.equal(got[~inf], want[~inf])                              # and the others exact and finite


# ---- 6. weight bank -------------------------------------------------------------------------------------------------------
def test_weight_bank_in_fp16():
    from mrla_amd import _lib as L, functional as Fm
    torch.manual_seed(5)
    convs = [torch.nn.Conv2d(k, n, 1, bias=False).cuda() for k, n in ((64, 256), (256, 64), (512, 2048), (128, 128))]
    convs[1].to(memory_format=CL)
    flat = lambda c: c.weight.detach().reshape(c.out_channels, c.in_channels)  # noqa: E731
    bank = Fm.WeightBank(convs)

    def fresh(dtype):
        torch.cuda.synchronize()
        return all(torch.equal(bank.get(c, dtype)[0], flat(c).to(dtype)) for c in convs)
    with torch.autocast("cuda", dtype=F16):
        bank.refresh()
    torch.cuda.synchronize()
    for c in convs:
        assert bank.get(c) is None and bank.get(c, torch.bfloat16) is None           # fp16 copies are not handed to a bf16 GEMM
        w16, w16t = bank.get(c, F16)
        assert w16.dtype == F16 and torch.equal(w16, flat(c).half()) and torch.equal(w16t, flat(c).half().t().contiguous())
    # without arguments, outside autocast: bf16, as ever (a change of dtype outside a capture rebuilds)
    old = bank.flat
    bank.refresh()
    assert bank.flat is not old and bank.flat.dtype == torch.bfloat16
    assert all(bank.get(c, F16) is None for c in convs) and fresh(torch.bfloat16)
    assert torch.equal(bank.get(convs[0])[1], flat(convs[0]).bfloat16().t().contiguous())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        keep = bank.flat
        bank.refresh()
        assert bank.flat is keep                                                     # same dtype: no rebuild
    bank.refresh(F16)                                                                # explicit dtype
    assert bank.flat.dtype == F16 and fresh(F16)
    # after an optimizer step a training forward re-casts
    opt = torch.optim.SGD([c.weight for c in convs], lr=0.5)
    for c in convs:
        c.weight.grad = torch.ones_like(c.weight)
    opt.step()
    assert not fresh(F16)
    with torch.autocast("cuda", dtype=F16):
        bank.refresh()
    assert fresh(F16)
    # a change of dtype inside a capture is refused like a first use (the table upload is not capturable)
    raised = []
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            try:
                bank.refresh(torch.bfloat16)
            except L.MrlaHipError as e:
                raised.append(str(e))
    except RuntimeError:
        pass                                                      # (an empty capture may itself be refused by the runtime)
    assert raised and "capture" in raised[0]
    assert bank.flat.dtype == F16 and fresh(F16)                  # untouched
    with pytest.raises(ValueError):
        bank.refresh(torch.float32)


# ---- 7. composite ---------------------------------------------------------------------------------------------------------
def _modules(k, n, wt):
    conv = torch.nn.Conv2d(k, n, 1, bias=False).cuda().to(memory_format=CL)
    bn = torch.nn.BatchNorm2d(n).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(wt).view(n, k, 1, 1))
        bn.weight.copy_(torch.from_numpy(1 + 0.2 * detgen.uniform((n,), 5)))
        bn.bias.copy_(torch.from_numpy(0.1 * detgen.uniform((n,), 6)))
    return conv, bn


def _reference(conv, bn, xt, gup, relu, g_through=None):
    """nn.Conv2d -> nn.BatchNorm2d -> relu in fp32 on the same fp16-rounded operands; the convolution output rounded to fp16
    where the product stores it."""
    k, n = conv.in_channels, conv.out_channels
    conv_r, bn_r = torch.nn.Conv2d(k, n, 1, bias=False).cuda(), torch.nn.BatchNorm2d(n).cuda()
    conv_r.load_state_dict(conv.state_dict()); bn_r.load_state_dict(bn.state_dict())
    bn_r.running_mean.zero_(); bn_r.running_var.fill_(1.0); bn_r.num_batches_tracked.zero_()
    xr = xt.detach().float().requires_grad_(True)
    zr = bn_r(conv_r(xr).half().float())
    if relu:
        zr = torch.relu(zr)
    if g_through is None:
        zr.backward(gup.float())
    else:
        torch.autograd.backward([zr, xr * 1.0], [gup.float(), g_through.float()])
    return conv_r, bn_r, xr, zr


@pytest.mark.parametrize("shape", [(4, 14, 14, 256, 64, True), (4, 14, 14, 64, 256, False), (3, 28, 28, 128, 512, False)],
                         ids=lambda s: "x".join(map(str, s)))
def test_conv_bn_act_composite_under_fp16_autocast(shape):
    """The shapes and bounds of tests/test_conv1x1_gpu.py::test_conv_bn_act_composite_matches_stock_modules (fp16 carries three
    more mantissa bits than bf16: conservative), with fp32 master weights and their fp16 working copies from the bank."""
    from mrla_amd import functional as Fm
    b, h, w, k, n, relu = shape
    x, wt = _operands(b, h, w, k, n, salt=1)
    conv, bn = _modules(k, n, wt)
    xt = torch.from_numpy(x).cuda().half().permute(0, 3, 1, 2).requires_grad_(True)
    gup = torch.from_numpy(f16_round(detgen.normalish((b, n, h, w), 9))).cuda().half().contiguous(memory_format=CL)
    bank = Fm.WeightBank([conv])
    Fm.TIMER = timer = Fm.KernelTimer(names=None)
    try:
        with torch.autocast("cuda", dtype=F16), Fm.batched_bookkeeping(0, bank.refresh()):
            assert Fm.conv1x1_applies(conv, xt) and bank.get(conv, F16) is not None
            out = Fm.conv_bn_act(xt, conv, bn, relu=relu)
        out.backward(gup)
        torch.cuda.synchronize()
    finally:
        Fm.TIMER = None
    assert {"mrla_conv1x1_fwd", "mrla_conv1x1_bwd_data", "mrla_conv1x1_wgrad"} <= set(timer.summary()), sorted(timer.summary())
    assert out.dtype == F16 and conv.weight.grad.dtype == torch.float32
    conv_r, bn_r, xr, zr = _reference(conv, bn, xt, gup, relu)
    a, r = out.detach().float(), zr.detach()
    bad = (a - r).abs() > 2.0 ** -7 * (r.abs() + 0.05 * r.abs().max())
    assert bad.float().mean().item() < 1e-4
    assert torch.allclose(bn.running_mean, bn_r.running_mean, rtol=1e-4, atol=1e-6)
    assert torch.allclose(bn.running_var, bn_r.running_var, rtol=1e-4, atol=1e-6)
    for name, got, want, tol in (("bn.weight", bn.weight.grad, bn_r.weight.grad, 2e-2), ("bn.bias", bn.bias.grad, bn_r.bias.grad, 2e-2),
                                 ("conv.weight", conv.weight.grad, conv_r.weight.grad, 3e-2), ("x", xt.grad.float(), xr.grad, 3e-2)):
        e = ((got.float() - want).norm() / want.norm()).item()
        print(f"{name}: gradient error {e:.3e} (bound {tol})")
        assert e < tol, name


def test_stride_1_shortcut_gradient_joins_the_fp16_input_gradient_gemm(monkeypatch):
    """conv1 with passthrough=True and a stride-1 shortcut: its input-gradient GEMM takes the shortcut's gradient as its addend
    (mrla_conv1x1_fwd_addend), and the sum is the stock modules' dX + that gradient."""
    from mrla_amd import _lib as L, functional as Fm
    b, h, w, k, n = 4, 14, 14, 256, 64
    x, wt = _operands(b, h, w, k, n, salt=6)
    conv, bn = _modules(k, n, wt)
    xt = torch.from_numpy(x).cuda().half().permute(0, 3, 1, 2).requires_grad_(True)
    g1 = torch.from_numpy(f16_round(detgen.normalish((b, n, h, w), 29))).cuda().half().contiguous(memory_format=CL)
    g2 = torch.from_numpy(f16_round(detgen.normalish((b, k, h, w), 31))).cuda().half().contiguous(memory_format=CL)
    entries, call = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (entries.append(name), call(name, *a))[1])
    with torch.autocast("cuda", dtype=F16):
        out, through = Fm.conv_bn_act(xt, conv, bn, relu=True, passthrough=True)
    assert through.data_ptr() == xt.data_ptr() and through.grad_fn is not None
    torch.autograd.backward([out, through], [g1, g2])
    torch.cuda.synchronize()
    assert "mrla_conv1x1_fwd_addend" in entries and "mrla_conv1x1_fwd" in entries and "mrla_conv1x1_wgrad" in entries
    conv_r, bn_r, xr, _ = _reference(conv, bn, xt, g1, True, g_through=g2)
    assert ((xt.grad.float() - xr.grad).norm() / xr.grad.norm()).item() < 3e-2
    assert ((conv.weight.grad - conv_r.weight.grad).norm() / conv_r.weight.grad.norm()).item() < 3e-2


# ---- 8. capture -----------------------------------------------------------------------------------------------------------
def test_captured_fp16_forward_and_backward_replays_the_eager_bits():
    from mrla_amd import functional as Fm
    b, h, w, k, n = 8, 14, 14, 64, 128
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(k, n, 1, bias=False).cuda().half().to(memory_format=CL)
    bn = torch.nn.BatchNorm2d(n).cuda()
    xs = torch.randn(b, k, h, w, device="cuda").half().contiguous(memory_format=CL).requires_grad_(True)
    gup = torch.randn(b, n, h, w, device="cuda").half().contiguous(memory_format=CL)
    assert Fm.conv1x1_applies(conv, xs)
    step = lambda: torch.autograd.grad(Fm.conv_bn_act(xs, conv, bn, relu=True), [xs, conv.weight], gup)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            gx, gw = step()
    torch.cuda.current_stream().wait_stream(side)
    want_x, want_w = gx.detach().clone(), gw.detach().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx_static, gw_static = step()
    for _ in range(3):             # the pool poisoned between replays: a kernel that relies on memory it found zeroed shows
        gx_static.fill_(float("nan")); gw_static.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gx_static, want_x) and torch.equal(gw_static, want_w)


# ---- 9. model -------------------------------------------------------------------------------------------------------------
def test_fp16_autocast_scaled_train_step_tracks_the_eager_restatement():
    """One GradScaler step (init_scale = 1024) of resnet50_mrlal at batch 8 under fp16 autocast vs the eager restatement from
    the same weights, at the bounds of tests/test_models_gpu.py::test_bf16_autocast_train_step_tracks_the_eager_restatement."""
    from oracle import eager_models as em
    from mrla_amd import functional as Fm, models
    from tests import cases
    from tests.test_models_gpu import load_det, rel
    net, ref = models.resnet50_mrlal().cuda(), em.eager_resnet50_mrlal().cuda()
    load_det(net)
    ref.load_state_dict(net.state_dict())
    net.train(); ref.train()
    x = torch.from_numpy(cases.image_batch(8, "img-train")).cuda()
    tgt = (torch.arange(8) * 37 % 1000).cuda()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    before = [p.detach().clone() for p in net.parameters()]
    labels = ["mrla_conv1x1_fwd", "mrla_conv1x1_bwd_data", "mrla_conv1x1_wgrad"]
    Fm.TIMER = timer = Fm.KernelTimer(labels)
    try:
        with torch.autocast("cuda", dtype=F16):
            y = net(x)
        la = torch.nn.functional.cross_entropy(y.float(), tgt)
        scaler.scale(la).backward()
        torch.cuda.synchronize()
    finally:
        Fm.TIMER = None
    with torch.autocast("cuda", dtype=F16):
        yr = ref(x)
    lb = torch.nn.functional.cross_entropy(yr.float(), tgt)
    (lb * 1024.0).backward()
    assert abs(la.item() - lb.item()) < 3e-2 * abs(lb.item())
    assert rel(y.detach().float().cpu().numpy(), yr.detach().float().cpu().numpy()) < 6e-2
    # the stride-1 1x1 convolutions ran on the GEMMs: 16 conv1 + 16 conv3 + the stride-1 downsample of stage 1, in all three roles
    launches = {k_: v["launches"] for k_, v in timer.summary().items()}
    print("GEMM launches:", launches)
    assert set(launches) == set(labels) and launches["mrla_conv1x1_fwd"] >= 33 and launches["mrla_conv1x1_wgrad"] >= 33
    assert launches["mrla_conv1x1_bwd_data"] >= 32
    scaler.unscale_(opt)
    dots = np.zeros(3)
    for (k_, pa), (_, pb) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.isfinite(pa.grad).all(), k_
        a, r = pa.grad.double().flatten(), pb.grad.double().flatten() / 1024.0
        dots += np.array([float(a @ r), float(a @ a), float(r @ r)])
    cosine = dots[0] / np.sqrt(dots[1] * dots[2])
    print(f"gradient cosine vs eager {cosine:.4f}")
    assert cosine > 0.8
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 1024.0                                       # a skipped step would have halved it
    assert any(not torch.equal(p.detach(), q) for p, q in zip(net.parameters(), before))
