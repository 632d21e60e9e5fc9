"""GPU: mrla_conv3x3_wgrad (mrla_amd/csrc/conv3x3_wgrad.hip) and its route in the Python layer at the shapes the DEFAULT
settings send to it -- functional.CONV3X3_WGRAD_AUTO is on, and an eligible stride-1 3x3 convolution takes its weight gradient
from the own kernel wherever mrla_conv3x3_wgrad_preferred answers 1: at least 384 output pixels per split and at least 4 steps
per workgroup, which for ResNet shapes means batch 64 and up.  The other conv3x3 test files stay below batch 18 (the C ABI) or
enter the explicit switch mrla_amd.conv3x3_wgrad() at batch 2 - 16 (the route); none of their shapes is a preferred one.

1. The kernel through the C ABI at the routed plan classes (SHAPES; the first test establishes every figure its comment claims
   through mrla_conv3x3_wgrad_plan / _preferred): many full-raster steps per workgroup, all four dY pieces and both X passes
   prefetched at every step, hundreds of splits, ranges that begin and end inside images.  Method and helpers of
   tests/test_conv3x3_wgrad_gpu.py: dyadic inputs give the float64 gradient bit for bit inside NaN-patterned guards, the
   partial tiles sum exactly to it; normal inputs stay inside the derived fp32 summation bound; a second call into dirty
   buffers and three replays of a captured call are bit-equal.
2. Non-finite inputs: what the kernel does with one +inf / NaN in dy or one +inf in x (NONFINITE_SHAPES, small: the contract
   does not depend on size).  Under fp16 autocast with a GradScaler an overflow has to show as a non-finite gradient.
3. The route under default switches, no switch context entered: functional.conv3x3 on a CUDA tensor (_conv3x3_own_wgrad, its
   shape cache _WGRAD_PREFERRED, _Conv3x3Fn with an fp32 master weight and with a 16-bit weight, _weight_strides for a weight
   that is not channels_last, what stays on the stock operator, a captured forward + backward).

The reference is always float64 on the CPU, never the kernel: nine float64 matmuls dY^T [n, P] @ X_shift [P, c] (_dw64_taps),
which tests/test_conv3x3_wgrad_prefetch_cpu.py holds equal to the autograd reference of tests/test_conv3x3_wgrad_gpu.py."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv3x3_route_gpu import ULP, _Counter
from tests.test_conv3x3_wgrad_gpu import DTYPES, UNIT, _Case, _bits, _ids, _inputs, _out_hw, _plan
from tests.test_conv3x3_wgrad_prefetch_gpu import MAX_KP, MAX_PY, _steps

pytestmark = pytest.mark.gpu
CL = torch.channels_last

# (b, c, n, h, w, s): per class the smallest batch at which the rule answers 1 (the first: the smallest with whole images per
# range); what test_the_shapes_are_of_the_routed_plan_classes asserts of each is written behind it
SHAPES = [
    (63, 512, 512, 7, 7, 1),     # 64 tiles, 8 splits of 56 rows, last range 49: 8 steps of 7 rows, one image each (layer 4)
    (67, 256, 256, 13, 14, 1),   # 16 tiles, 32 splits of 28 rows, rmax 8, last range 3 rows: image borders at odd places
    (62, 128, 128, 27, 28, 1),   # 4 tiles, 120 splits of 14 rows, rmax 4, last range 8: KP = 120 of the 128-row raster
    (56, 64, 64, 55, 56, 1),     # 1 tile, 440 splits of 7 rows, rmax 2, pitch 58, 4 steps; 55 is no multiple of 7
    (43, 64, 256, 6, 131, 1),    # 4 tiles, 86 splits of 3 rows, column segments 58, 58, 15: 9 steps; n != c
]
EXPECTED = {                     # shape -> (tiles, splits, rows per split, rmax, rows of the last range, steps of a full range)
    SHAPES[0]: (64, 8, 56, 7, 49, 8),
    SHAPES[1]: (16, 32, 28, 8, 3, None),          # (4 to 6 steps: the image borders fall differently in every range)
    SHAPES[2]: (4, 120, 14, 4, 8, None),
    SHAPES[3]: (1, 440, 7, 2, 7, 4),
    SHAPES[4]: (4, 86, 3, 1, 3, 9),
}
PREFER_STEPS, PREFER_PIXELS = 4, 384              # conv3x3_wgrad.hip: kC3PreferSteps, kC3PreferPixels
NONFINITE_SHAPES = [(2, 64, 128, 7, 7, 1), (2, 64, 64, 9, 6, 2)]
ROUTED = [(64, 512, 512, 7, 7, 1), (43, 64, 256, 6, 131, 1)]
BELOW = [(54, 512, 512, 7, 7, 1), (61, 512, 512, 7, 7, 1)]    # 48 and 54 rows per split: 336 and 378 pixels (62 is the first with 385)


def _rmax_nseg(shape):
    """Rows per step and column segments per row, by conv_spatial.h's raster rule."""
    b, c, n, h, w, s = shape
    wo = _out_hw(h, w, s)[1]
    pad = 2 if s == 1 else 1
    if wo + pad <= MAX_PY:
        return max(1, min(_out_hw(h, w, s)[0], MAX_KP[s] // (wo + pad))), 1
    return 1, -(-wo // (MAX_PY - pad))


def _dw64_taps(x, dy, s):
    """The float64 weight gradient [n, 3, 3, c] of conv2d(x, w, stride s, padding 1) as nine matmuls dY^T [n, P] @ X_shift [P, c]."""
    b, c, h, w = x.shape
    n, (ho, wo) = dy.shape[1], dy.shape[2:]
    assert x.dtype == dy.dtype == torch.float64 and (ho, wo) == _out_hw(h, w, s)
    xp = F.pad(x, (1, 1, 1, 1))
    dyt = dy.permute(1, 0, 2, 3).reshape(n, -1)
    out = torch.empty((n, 3, 3, c), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xp[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]
            out[:, kh, kw, :] = dyt @ xs.permute(0, 2, 3, 1).reshape(-1, c)
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dname="bf16"):
    """(dw64, A) [n, 3, 3, c] of tests/test_conv3x3_wgrad_gpu.py's _inputs: the float64 gradient and the same gradient of |x|,
    |dy|.  Computed once per case, never modified."""
    x, dy = _inputs(shape, kind, dname)
    return _dw64_taps(x, dy, shape[5]), _dw64_taps(x.abs(), dy.abs(), shape[5])


def _summation_bound(m, a, want64, dw_dtype):
    """(m + 9) * 2^-24 * A + u * |dw64| of tests/test_conv3x3_wgrad_gpu.py, with its fp16 subnormal clause."""
    store = UNIT[dw_dtype] * want64.abs()
    if dw_dtype == torch.float16:
        store = torch.where(want64.abs() < 2.0 ** -14, torch.full_like(store, 2.0 ** -25), store)
    return (m + 9) * 2.0 ** -24 * a + store


# ---------------------------------------------------------------- 1. the kernel at the routed plan classes

def test_the_shapes_are_of_the_routed_plan_classes():
    from mrla_amd import _lib as L
    pref = L.load().mrla_conv3x3_wgrad_preferred
    inside = 0
    for shape in SHAPES:
        b, c, n, h, w, s = shape
        ho, wo = _out_hw(h, w, s)
        tiles, splits, per, rmax, last, full = EXPECTED[shape]
        for dt in (L.BF16, L.F16):
            assert pref(*shape, dt) == 1, shape
            plan = _plan(shape, dt)
            assert (plan[5], plan[4], plan[2]) == (tiles, splits, per), (shape, plan)
        assert _rmax_nseg(shape)[0] == rmax and b * ho - (splits - 1) * per == last, shape
        # the rule's own quantities, and the steps a workgroup really walks (more where an image border cuts a step short);
        # the last, shorter range may have fewer
        assert -(-per // rmax) * _rmax_nseg(shape)[1] >= PREFER_STEPS and per * wo >= PREFER_PIXELS, shape
        steps = _steps(shape, L.BF16)
        assert len(steps) == splits and all(len(st) >= PREFER_STEPS for st in steps[:-1]), shape
        assert sum(r for st in steps for r, _ in st) == b * ho * _rmax_nseg(shape)[1], shape
        if full is not None:
            assert {len(st) for st in steps[:-1]} == {full}, shape
        inside += any((i * per) % ho for i in range(1, splits))
    assert inside >= 3                                                    # a split boundary strictly inside an image
    assert _steps(SHAPES[0], L.BF16)[0] == [(7, 7)] * 8                   # one image per step
    assert _steps(SHAPES[1], L.BF16)[0] == [(8, 14), (5, 14), (8, 14), (5, 14), (2, 14)] and _steps(SHAPES[1], L.BF16)[-1] == [(3, 14)]
    assert _steps(SHAPES[2], L.BF16)[0] == [(4, 28)] * 3 + [(2, 28)] and (4 * 30 + 15) & ~15 == 128       # KP 120 -> 128 rows
    assert _steps(SHAPES[3], L.BF16)[0] == [(2, 56)] * 3 + [(1, 56)]
    assert _steps(SHAPES[4], L.BF16)[0] == [(1, 58), (1, 58), (1, 15)] * 3
    for shape in ROUTED:
        assert pref(*shape, L.BF16) == 1 and pref(*shape, L.F16) == 1, shape
    for shape in BELOW + [(64, 512, 512, 14, 14, 2)]:
        assert pref(*shape, L.BF16) == 0 and pref(*shape, L.F16) == 0, shape
    assert pref(62, 512, 512, 7, 7, 1, L.BF16) == 1                       # BELOW[1] is one batch below the threshold


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_inputs_give_the_float64_gradient_bit_for_bit_and_the_partial_tiles_sum_to_it(shape, dname, wide):
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    want64, a = _reference(shape, "dyadic")
    # exactness of every fp32 partial sum, in any order: multiples of 1/8 bounded by the sum of the magnitudes
    assert float(a.max()) * 8 < 2 ** 24 and torch.equal((want64 * 8).round(), want64 * 8)
    want = (want64 + 0.0).float().to(dw_dtype)
    assert torch.equal(want64.float().double(), want64)
    case = _Case(shape, "dyadic", dname, dw_dtype)
    case.launch()
    dw, part = case.results()                                # (NaN-pattern-free payloads, untouched guards: _Guarded.check_output)
    bad = _bits(dw) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(part.double().view(case.rows, -1).sum(0), want64.reshape(-1))


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_normal_inputs_stay_inside_the_fp32_summation_bound(shape, dname, wide):
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    want64, a = _reference(shape, "normal", dname)
    case = _Case(shape, "normal", dname, dw_dtype)
    case.launch()
    dw, _ = case.results()
    m = b * ho * wo
    err = (dw.double() - want64).abs()
    ratio = float((err / a.clamp_min(1e-300)).max())
    print(f"{shape} {dname} dw {dw_dtype}: max |dw - dw64| / A = {ratio:.3e} (fp32 term of the bound {(m + 9) * 2.0 ** -24:.3e})")
    bound = _summation_bound(m, a, want64, dw_dtype)
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_a_second_call_into_dirty_buffers_and_three_replays_are_bit_equal(shape):
    case = _Case(shape, "normal", "bf16", torch.float32)
    case.launch()
    dw0, part0 = case.results()
    want64, a = _reference(shape, "normal", "bf16")
    assert float(((dw0.double() - want64).abs() / a.clamp_min(1e-300)).max()) < 1e-3      # (the first call is the right answer)
    case.gpart.payload.fill_(3.0)
    case.gdw.payload.fill_(-7.0)
    case.launch()
    torch.cuda.synchronize()
    assert torch.equal(_bits(case.gdw.payload.cpu().view_as(dw0)), _bits(dw0)), "second call: dw differs"
    assert torch.equal(_bits(case.gpart.payload.cpu()), _bits(part0)), "second call: part differs"
    case.refill_outputs()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            case.launch()
    for i in range(3):
        case.refill_outputs()
        graph.replay()
        dw, part = case.results()
        assert torch.equal(_bits(dw), _bits(dw0)), f"replay {i}: dw differs from the first call"
        assert torch.equal(_bits(part), _bits(part0)), f"replay {i}: part differs from the first call"


# ---------------------------------------------------------------- 2. non-finite inputs

@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=_ids)
def test_one_non_finite_input_element_poisons_its_own_row_or_column_and_nothing_else(shape, dname, wide):
    """One +inf or NaN in dy at output channel n0, or one +inf in x at input channel c0, at an interior pixel of image 1.

    The float64 reference (the same nine matmuls on the same poisoned tensors) gives +-inf or NaN at exactly the elements of
    dw[n0] / dw[:, :, :, c0] whose tap reads the pixel: all nine taps of every c (every n) at stride 1 and for dy at stride 2;
    for x at stride 2 only the taps whose parity meets the pixel, and it keeps every other element finite.  The kernel must be
    non-finite at every such element, and every OTHER row (column) must be bit-equal to the call on the clean inputs: rows and
    columns of the product are independent, so a NaN anywhere else is an operand read from the wrong place.  Inside the
    poisoned row / column the kernel may be non-finite where the reference is finite, and NaN where the reference is +-inf:
    the rasters' pad pixels are zeros that the MFMA multiplies like any pixel, and 0 * inf = NaN, where the reference has no
    such product.  An overflow can therefore not vanish; it can only spread inside its own row or column."""
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    x64, dy64 = _inputs(shape, "normal", dname)
    case = _Case(shape, "normal", dname, dw_dtype)
    case.launch()
    dw0, part0 = case.results()
    part0 = part0.view(case.rows, n, 3, 3, c)
    assert bool(torch.isfinite(dw0.float()).all()) and bool(torch.isfinite(part0).all())
    n0, c0 = n - 27, 21
    yo, xo, yi, xi = ho // 2, wo // 2, h // 2, w // 2
    assert 0 < yo < ho - 1 and 0 < xo < wo - 1 and s * yo + 1 < h and s * xo + 1 < w and 0 < yi < h - 1 and 0 < xi < w - 1
    dy_dev, x_dev = case.gdy.payload.view(b, ho, wo, n), case.gx.payload.view(b, h, w, c)
    for what, value in (("dy", float("inf")), ("dy", float("nan")), ("x", float("inf"))):
        xq, dyq = x64.clone(), dy64.clone()
        if what == "dy":
            dyq[1, n0, yo, xo] = value
            keep, was = (1, yo, xo, n0), dy_dev[1, yo, xo, n0].clone()
            dy_dev[keep] = value
        else:
            xq[1, c0, yi, xi] = value
            keep, was = (1, yi, xi, c0), x_dev[1, yi, xi, c0].clone()
            x_dev[keep] = value
        ref_bad = ~torch.isfinite(_dw64_taps(xq, dyq, s))                 # [n, 3, 3, c]
        own = torch.zeros_like(ref_bad)
        if what == "dy":
            own[n0] = True
            assert bool(ref_bad[n0].all())                               # all nine taps, every c
        else:
            own[..., c0] = True
            # tap (kh, kw) reads input pixel (yi, xi) at output pixel ((yi + 1 - kh) / s, (xi + 1 - kw) / s), where that is one
            reads = torch.tensor([[(yi + 1 - kh) % s == 0 and (yi + 1 - kh) // s < ho and (xi + 1 - kw) % s == 0 and (xi + 1 - kw) // s < wo
                                   for kw in range(3)] for kh in range(3)])
            assert int(reads.sum()) == (9 if s == 1 else 2)              # (stride 2: an even row, an odd column)
            assert torch.equal(ref_bad[..., c0], reads.expand(n, 3, 3))  # the same taps for every n
        assert not bool((ref_bad & ~own).any())                          # the reference: nothing outside the row / column
        case.new_outputs()
        case.launch()
        dw, part = case.results()
        part = part.view(case.rows, n, 3, 3, c)
        (dy_dev if what == "dy" else x_dev)[keep] = was                   # (clean again for the next round)
        tag = f"{what} = {value}"
        got_bad = ~torch.isfinite(dw.float())
        assert bool(got_bad[ref_bad].all()), f"{tag}: {int((ref_bad & ~got_bad).sum())} elements finite where float64 is not"
        assert torch.equal(_bits(dw)[~own], _bits(dw0)[~own]), f"{tag}: dw differs from the clean call outside the row / column"
        # part: the same pattern -- some split non-finite wherever float64 is, everything else the clean call's bits
        part_bad = ~torch.isfinite(part)
        assert bool(part_bad.any(0)[ref_bad].all()), f"{tag}: part finite in every split where float64 is not"
        outside = ~own.expand_as(part_bad)
        assert torch.equal(_bits(part)[outside], _bits(part0)[outside]), f"{tag}: part differs outside the row / column"
    torch.cuda.synchronize()
    case.new_outputs()                                                   # the inputs are what they were: the clean result again
    case.launch()
    assert torch.equal(_bits(case.results()[0]), _bits(dw0))


# ---------------------------------------------------------------- 3. the route under default switches

def _defaults():
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_WGRAD_AUTO is True and Fm.CONV3X3_WGRAD is False
    return Fm


@contextlib.contextmanager
def _deterministic():
    was = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    try:
        yield
    finally:
        torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = was


def _conv(c, n, s=1, channels_last=True):
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(c, n, 3, stride=s, padding=1, bias=False).cuda()
    return conv.to(memory_format=CL) if channels_last else conv


def _data(shape, dtype):
    b, c, n, h, w, s = shape
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((b, c, h, w), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    dy = torch.randn((b, n, *_out_hw(h, w, s)), device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    return x, dy


@functools.lru_cache(maxsize=None)
def _route_reference(shape, dtype):
    """(dw64, A) as [n, c, 3, 3] for _data(shape, dtype)."""
    x, dy = _data(shape, dtype)
    x64, dy64 = x.double().cpu(), dy.double().cpu()
    return tuple(t.permute(0, 3, 1, 2) for t in (_dw64_taps(x64, dy64, shape[5]), _dw64_taps(x64.abs(), dy64.abs(), shape[5])))


def _direct(shape, dtype, x, dy, dw_dtype=torch.float32):
    """The C ABI on the same x, dy: dw as a channels_last [n, c, 3, 3]."""
    from mrla_amd import _lib as L, functional as Fm
    b, c, n, h, w, s = shape
    rows = L.load().mrla_conv3x3_wgrad_rows(*shape, Fm._DT[dtype])
    part = torch.empty((rows, n, 9, c), dtype=torch.float32, device="cuda")
    dw = torch.empty((n, c, 3, 3), dtype=dw_dtype, device="cuda", memory_format=CL)
    L.call("mrla_conv3x3_wgrad", dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), *shape, Fm._DT[dtype],
           Fm._DT[dw_dtype], Fm._stream())
    return dw


def _assert_same_as_unrouted(name, got, want, dtype):
    """The project's criterion between two calls of the stock operator (tests/test_conv3x3_route_gpu.py): 2 ulps of the 16-bit
    type at the tensor's largest magnitude.  Both sides run under cudnn.deterministic."""
    err = float((got.double() - want.double()).abs().max())
    tol = 2 * ULP[dtype] * float(want.double().abs().max())
    print(f"{name}: routed against unrouted {err:.3e}, 2 ulps at the largest magnitude {tol:.3e}")
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", ROUTED, ids=_ids)
def test_default_switches_route_a_preferred_shape_and_the_fp32_gradient_is_the_kernels(shape, dtype, monkeypatch):
    import mrla_amd
    Fm = _defaults()
    count = _Counter(monkeypatch)
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    ours, stock = _conv(c, n, s), _conv(c, n, s)
    assert torch.equal(ours.weight, stock.weight) and ours.weight.dtype == torch.float32
    x0, dy = _data(shape, dtype)
    xo, xs = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    with _deterministic():
        with torch.autocast("cuda", dtype=dtype):
            yo = Fm.conv3x3(xo, ours)
            with mrla_amd.conv3x3_wgrad_auto(False):
                ys = Fm.conv3x3(xs, stock)
                assert type(ys.grad_fn).__name__ == type(stock(xs).grad_fn).__name__          # ... which is conv(x) itself
        assert type(yo.grad_fn).__name__.startswith("_Conv3x3Fn") and yo.dtype == dtype and yo.shape == ys.shape
        assert not type(ys.grad_fn).__name__.startswith("_Conv3x3Fn")
        ys.backward(dy)
        assert count.n == 0
        yo.backward(dy, retain_graph=True)
        assert count.n == 1
        _assert_same_as_unrouted("out", yo.detach(), ys.detach(), dtype)
        _assert_same_as_unrouted("dx", xo.grad, xs.grad, dtype)
    gw = ours.weight.grad
    assert gw.dtype == torch.float32 and gw.shape == (n, c, 3, 3) and gw.stride() == ours.weight.stride()
    want64, a = _route_reference(shape, dtype)
    err = (gw.double().cpu() - want64).abs()
    print(f"{shape} {dtype}: max |dw - dw64| / A = {float((err / a.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= (b * ho * wo + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max())
    assert torch.equal(_bits(gw), _bits(_direct(shape, dtype, x0, dy)))                     # the C ABI on the same x, dy
    first = gw.clone()
    ours.weight.grad = None
    yo.backward(dy, retain_graph=True)                                                    # a second backward
    assert count.n == 2 and torch.equal(_bits(ours.weight.grad), _bits(first))
    yo.backward(dy)                                                                       # ... and a third, accumulated: x + x is exact
    assert count.n == 3 and torch.equal(_bits(ours.weight.grad), _bits(first + first))
    assert ours.weight.grad.stride() == ours.weight.stride()


@pytest.mark.parametrize("shape", ROUTED, ids=_ids)
def test_a_16_bit_weight_without_autocast_gets_its_gradient_rounded_once(shape, monkeypatch):
    Fm = _defaults()
    count = _Counter(monkeypatch)
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    dtype = torch.bfloat16
    conv = _conv(c, n, s).bfloat16()
    x0, dy = _data(shape, dtype)
    x = x0.clone().requires_grad_(True)
    y = Fm.conv3x3(x, conv)
    assert type(y.grad_fn).__name__.startswith("_Conv3x3Fn") and y.dtype == dtype
    y.backward(dy, retain_graph=True)
    gw = conv.weight.grad
    assert count.n == 1 and gw.dtype == dtype and gw.shape == (n, c, 3, 3) and gw.stride() == conv.weight.stride()
    want64, a = _route_reference(shape, dtype)
    err = (gw.double().cpu() - want64).abs()
    bound = _summation_bound(b * ho * wo, a, want64, dtype)
    print(f"{shape} bf16 weight: max |dw - dw64| / A = {float((err / a.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"
    assert torch.equal(_bits(gw), _bits(_direct(shape, dtype, x0, dy, dtype)))
    first = gw.clone()
    conv.weight.grad = None
    y.backward(dy)
    assert count.n == 2 and torch.equal(_bits(conv.weight.grad), _bits(first))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", ROUTED, ids=_ids)
def test_a_weight_in_contiguous_strides_gets_the_same_gradient_in_its_own_strides(shape, dtype, monkeypatch):
    """_weight_strides: the kernel writes [n, 3, 3, c]; a weight in NCHW strides (a DDP bucket view is one) must get the same
    numbers in ITS layout -- autograd's and DDP's layout contract."""
    Fm = _defaults()
    count = _Counter(monkeypatch)
    b, c, n, h, w, s = shape
    x0, dy = _data(shape, dtype)
    grads = []
    for channels_last in (True, False):
        conv = _conv(c, n, s, channels_last)
        assert conv.weight.is_contiguous() != channels_last and conv.weight.is_contiguous(memory_format=CL) == channels_last
        handed = []                                          # what the node hands to autograd, in front of any accumulation
        conv.weight.register_hook(lambda g: handed.append((g.stride(), g.dtype)))
        with torch.autocast("cuda", dtype=dtype):
            y = Fm.conv3x3(x0, conv)
        assert type(y.grad_fn).__name__.startswith("_Conv3x3Fn")
        y.backward(dy)
        gw = conv.weight.grad
        assert handed == [(conv.weight.stride(), torch.float32)], handed
        assert gw.dtype == torch.float32 and gw.shape == (n, c, 3, 3) and gw.stride() == conv.weight.stride()
        grads.append(gw)
    assert count.n == 2 and grads[0].stride() != grads[1].stride()
    assert torch.equal(_bits(grads[1]), _bits(grads[0]))                  # (as tensors: _bits goes through .contiguous())
    want64, a = _route_reference(shape, dtype)
    err = (grads[1].double().cpu() - want64).abs()
    assert bool((err <= (b * _out_hw(h, w, s)[0] * _out_hw(h, w, s)[1] + 9) * 2.0 ** -24 * a).all())


def _stock_name(conv, x, dtype):
    with torch.autocast("cuda", dtype=dtype):
        return type(conv(x).grad_fn).__name__


def test_below_the_threshold_stride_2_a_frozen_weight_and_no_grad_stay_on_the_stock_operator(monkeypatch):
    import mrla_amd
    Fm = _defaults()
    count = _Counter(monkeypatch)
    dtype = torch.bfloat16
    preferred = ROUTED[0]

    def run(shape, ctx=contextlib.nullcontext(), freeze=False):
        b, c, n, h, w, s = shape
        conv = _conv(c, n, s)
        conv.weight.requires_grad_(not freeze)
        x0, dy = _data(shape, dtype)
        x = x0.clone().requires_grad_(True)
        with ctx, torch.autocast("cuda", dtype=dtype):
            y = Fm.conv3x3(x, conv)
            assert torch.equal(y, conv(x))
        assert type(y.grad_fn).__name__ == _stock_name(conv, x, dtype) and not type(y.grad_fn).__name__.startswith("_Conv3x3Fn")
        y.backward(dy)
        assert count.n == 0, shape
        assert x.grad is not None and (conv.weight.grad is None) == freeze

    with _deterministic():                                   # (two calls of the stock forward are compared for equality)
        for shape in BELOW:                                  # 54, and 61: one batch below the threshold
            run(shape)
        run((64, 512, 512, 14, 14, 2))                       # stride 2
        run(preferred, ctx=mrla_amd.conv3x3_wgrad_auto(False))
        run(preferred, freeze=True)
        conv = _conv(512, 512)
        x0, _ = _data(preferred, dtype)
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            y = Fm.conv3x3(x0, conv)
            assert y.grad_fn is None and not y.requires_grad and torch.equal(y, conv(x0))
    assert count.n == 0


def test_the_shape_cache_holds_one_entry_per_shape_and_dtype_asked():
    import mrla_amd
    from mrla_amd import _lib as L
    Fm = _defaults()
    saved = dict(Fm._WGRAD_PREFERRED)
    Fm._WGRAD_PREFERRED.clear()
    try:
        asked = [(ROUTED[0], torch.bfloat16), (ROUTED[0], torch.bfloat16), (ROUTED[0], torch.float16), (ROUTED[1], torch.bfloat16),
                 (BELOW[0], torch.bfloat16), (BELOW[1], torch.float16), (BELOW[0], torch.bfloat16)]
        for shape, dtype in asked:
            b, c, n, h, w, s = shape
            conv, (x, _) = _conv(c, n, s), _data(shape, dtype)
            with torch.autocast("cuda", dtype=dtype):
                routed = type(Fm.conv3x3(x, conv).grad_fn).__name__.startswith("_Conv3x3Fn")
            assert routed == (shape in ROUTED)
        want = {(*shape, Fm._DT[dtype]): shape in ROUTED for shape, dtype in asked}
        assert len(want) == 5 and Fm._WGRAD_PREFERRED == want
        assert all(type(v) is bool for v in Fm._WGRAD_PREFERRED.values())
        # not asked: with the switch off, for a frozen weight, under no_grad (none of them reaches the query)
        conv, (x, _) = _conv(128, 128), _data((62, 128, 128, 27, 28, 1), torch.bfloat16)
        assert L.load().mrla_conv3x3_wgrad_preferred(62, 128, 128, 27, 28, 1, L.BF16) == 1
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with mrla_amd.conv3x3_wgrad_auto(False):
                Fm.conv3x3(x, conv)
            with torch.no_grad():
                Fm.conv3x3(x, conv)
            conv.weight.requires_grad_(False)
            Fm.conv3x3(x, conv)
        assert Fm._WGRAD_PREFERRED == want
    finally:
        Fm._WGRAD_PREFERRED.clear()
        Fm._WGRAD_PREFERRED.update(saved)


def test_replays_of_a_captured_forward_and_backward_give_the_eager_gradient(monkeypatch):
    Fm = _defaults()
    count = _Counter(monkeypatch)
    shape, dtype = ROUTED[0], torch.bfloat16
    b, c, n, h, w, s = shape
    conv = _conv(c, n, s)
    x0, dy = _data(shape, dtype)
    x = x0.clone().requires_grad_(True)

    def step():
        with torch.autocast("cuda", dtype=dtype):
            y = Fm.conv3x3(x, conv)
        assert type(y.grad_fn).__name__.startswith("_Conv3x3Fn")
        y.backward(dy)

    with _deterministic():
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            step()                                           # the eager warm-up, on the stream of the capture
        stream.synchronize()
        eager = conv.weight.grad.clone()
        want64, a = _route_reference(shape, dtype)
        assert bool(((eager.double().cpu() - want64).abs() <= (b * h * w + 9) * 2.0 ** -24 * a).all())
        assert torch.equal(_bits(eager), _bits(_direct(shape, dtype, x0, dy)))
        conv.weight.grad, x.grad = None, None
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                step()
        assert count.n == 2
        captured = conv.weight.grad
        assert captured is not None and captured.dtype == torch.float32 and captured.stride() == conv.weight.stride()
        for i in range(3):
            captured.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(captured), _bits(eager)), f"replay {i}: weight.grad differs from the eager one"
    assert count.n == 2
