"""GPU: mrla_conv3x3_fwd (mrla_amd/csrc/conv3x3_fwd.hip) through the C ABI against float64 on the CPU -- F.conv2d(x64, w64,
stride=s, padding=1) for the forward, aten.convolution_backward for the stride-1 input gradient the same entry point forms on
the flipped, transposed weight.

1. Exact: integer-valued x in [-4, 4] and wt in [-2, 2]: every fp32 partial sum is an integer below 9 * 512 * 8 < 2^24, exact
   in ANY order, so y must equal the float64 convolution cast once to the dtype, bit for bit.  y and mom_part sit inside
   NaN-patterned guards (untouched afterwards, no payload element left unwritten), x and wt inside guards of 2^14 (a read
   outside them breaks the equality).
2. Normal data rounded to the dtype first: |y - y64| <= u |y64| + (1 + u) 9c 2^-24 A + t, A = conv2d(|x|, |wt|) in float64
   (any summation order of 9c terms in fp32, then ONE rounding of relative size u = 2^-8 bf16, 2^-11 fp16; t = half the
   smallest subnormal, where the format is a fixed grid).  Derived, not measured; the measured maximum is printed.
3. Moments: per channel the counts sum to b*ho*wo, the raw sums rebuilt in float64 from the records agree with the float64
   sums of the STORED y, mom_part = NULL gives the same y bit for bit, and mrla_bn_stats_fwd_rows on the records gives the
   batch statistics of the stored y -- also where the mean is far above sigma (all-positive x and wt).
4. Determinism: further calls into fresh NaN-patterned buffers and into buffers that held ordinary numbers are bit-equal.
5. Replay: three replays of a captured call (y and mom_part overwritten with the NaN pattern in between) equal the eager call.
6. The input gradient at stride 1 through the same entry point: bit-equal on the integer data, the bound of item 2 with 9n
   terms on normal data."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv1x1_gpu import raw_sums
from tests.test_light_gpu import relmax
from tests.test_stem_exact_gpu import INT_OF, _Guarded, _bits, _nhwc

pytestmark = pytest.mark.gpu

SHAPES = [                       # (b, c, n, h, w, s)
    (1, 64, 64, 1, 1, 1),        # smallest stride-1 case: only the centre tap meets a pixel
    (1, 64, 64, 2, 1, 2),        # smallest stride-2 case
    (1, 64, 64, 3, 5, 1),        # small map, several rows in one step
    (2, 64, 128, 7, 7, 1),       # 7x7 map, two images, two n tiles
    (3, 128, 64, 8, 33, 1),      # rows of 33 pixels, c != n
    (2, 64, 64, 7, 7, 2),        # odd map at stride 2
    (2, 64, 64, 9, 6, 2),        # non-square map at stride 2
    (1, 128, 128, 14, 14, 2),    # several steps at stride 2
    (2, 256, 256, 14, 14, 1),    # several c-chunks
    (5, 64, 64, 28, 28, 1),      # a row range that crosses an image boundary
    (2, 512, 512, 7, 7, 1),      # eight c-chunks
    (1, 64, 64, 2, 70, 1),       # a row wider than a segment
    (1, 64, 64, 3, 131, 2),      # a row wider than a segment, stride 2
]
REPLAY_SHAPES = [(2, 512, 512, 7, 7, 1), (1, 128, 128, 14, 14, 2)]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}       # half the smallest subnormal
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _plan(shape, dt):
    from mrla_amd import _lib as L
    b, c, n, h, w, s = shape
    plan = L.conv3x3_fwd_plan(b, c, n, h, w, s, dt)
    rows = L.load().mrla_conv3x3_fwd_rows(b, c, n, h, w, s, dt)
    assert plan is not None and rows == plan[4] > 0
    return plan


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, dname="bf16"):
    """float64 CPU tensors x [b, c, h, w] and wt [n, c, 3, 3]: integers, or normal data rounded to the dtype, or all positive."""
    b, c, n, h, w, s = shape
    gen = torch.Generator().manual_seed(100000 * s + 1000 * h + 10 * w + c + n + b + {"int": 0, "normal": 7, "positive": 13}[kind])
    if kind == "int":
        x = torch.randint(-4, 5, (b, c, h, w), generator=gen).double()
        wt = torch.randint(-2, 3, (n, c, 3, 3), generator=gen).double()
    elif kind == "normal":
        x = torch.randn((b, c, h, w), generator=gen).to(DTYPES[dname]).double()
        wt = (torch.randn((n, c, 3, 3), generator=gen) * (2.0 / (9 * c)) ** 0.5).to(DTYPES[dname]).double()
    else:       # y ~ mean_n * (1 + 0.6 %): the centre tap carries the mean, the other eight 2^-9 of it (so borders barely show)
        x = (1.0 + 0.05 * torch.randn((b, c, h, w), generator=gen)).to(DTYPES[dname]).double()
        means = 64 + 56 * torch.rand((n,), generator=gen)
        wt = (means[:, None, None, None] / c * 2.0 ** -9).expand(n, c, 3, 3).clone()
        wt[:, :, 1, 1] = means[:, None] / c
        wt = wt.to(DTYPES[dname]).double()
        assert bool((x > 0).all()) and bool((wt > 0).all())
    return x, wt


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dname="bf16"):
    """(y64, A) [b, n, ho, wo]: the float64 convolution and the same of |x|, |wt|.  Computed once per case, never modified."""
    x, wt = _inputs(shape, kind, dname)
    s = shape[5]
    return F.conv2d(x, wt, stride=s, padding=1), F.conv2d(x.abs(), wt.abs(), stride=s, padding=1)


class _Case:
    """The guarded device buffers of one forward call, and the call."""

    def __init__(self, shape, kind, dname, moments=True):
        from mrla_amd import functional as Fm
        self.shape, self.dtype, self.moments = shape, DTYPES[dname], moments
        self.dt = Fm._DT[self.dtype]
        b, c, n, h, w, s = shape
        self.ho, self.wo = _out_hw(h, w, s)
        x, wt = _inputs(shape, kind, dname)
        self.rows = _plan(shape, self.dt)[4]
        self.gx = _Guarded(x.numel(), h * w * c, self.dtype, _nhwc(x))
        self.gw = _Guarded(wt.numel(), 9 * c, self.dtype, _nhwc(wt))          # [n, 3, 3, c]
        self.new_outputs()

    def new_outputs(self):
        b, c, n, h, w, s = self.shape
        self.gy = _Guarded(b * self.ho * self.wo * n, self.wo * n, self.dtype)
        self.gmom = _Guarded(self.rows * n * 4, n * 4, torch.float32)

    def refill_outputs(self):
        for g in (self.gy, self.gmom):
            g.flat.view(INT_OF[g.dtype]).fill_(g._pattern())

    def launch(self):
        from mrla_amd import _lib as L, functional as Fm
        b, c, n, h, w, s = self.shape
        L.call("mrla_conv3x3_fwd", self.gx.ptr(), self.gw.ptr(), self.gy.ptr(), self.gmom.ptr() if self.moments else None,
               b, c, n, h, w, s, self.dt, Fm._stream())

    def results(self):
        """(y [b, n, ho, wo], mom [rows, n, 4] or None) on the CPU, after the guard checks."""
        torch.cuda.synchronize()
        b, c, n, h, w, s = self.shape
        y = self.gy.check_output("y").view(b, self.ho, self.wo, n).permute(0, 3, 1, 2)
        mom = self.gmom.check_output("mom_part").view(self.rows, n, 4) if self.moments else None
        return y, mom


def test_the_cases_cover_what_they_are_for():
    """Through the plan: a row cut into segments, several steps in a workgroup, a row range over two images, several
    c-chunks, several record rows."""
    from mrla_amd import _lib as L
    segments = steps = spans = chunks = records = False
    for shape in SHAPES:
        b, c, n, h, w, s = shape
        tn, per, rstep, nseg, rows, wgs = _plan(shape, L.BF16)
        ho = _out_hw(h, w, s)[0]
        assert rows == -(-b * ho // per) and wgs == rows * (n // tn) and rstep >= 1 and nseg >= 1
        segments |= nseg > 1
        for i in range(rows):
            lo, hi = i * per, min(b * ho, (i + 1) * per)
            # steps of a range: rows of one image, at most rstep at a time
            nsteps, r = 0, lo
            while r < hi:
                r += min(rstep, ho - r % ho, hi - r)
                nsteps += 1
            steps |= nsteps * nseg > 1
            spans |= lo // ho != (hi - 1) // ho
        chunks |= c > 64
        records |= rows > 1
    assert segments and steps and spans and chunks and records


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_integer_inputs_give_the_float64_convolution_bit_for_bit_inside_guards(shape, dname):
    want64, a = _reference(shape, "int")
    assert float(a.max()) < 2 ** 24 and torch.equal(want64.round(), want64)
    want = (want64 + 0.0).float().to(DTYPES[dname])
    case = _Case(shape, "int", dname)
    case.launch()
    y, mom = case.results()
    if shape == (1, 64, 64, 1, 1, 1):
        x, wt = _inputs(shape, "int")
        assert torch.equal(want64[0, :, 0, 0], wt[:, :, 1, 1] @ x[0, :, 0, 0])
    bad = _bits(y) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_normal_inputs_stay_inside_the_fp32_summation_bound(shape, dname):
    b, c, n, h, w, s = shape
    dtype = DTYPES[dname]
    want64, a = _reference(shape, "normal", dname)
    case = _Case(shape, "normal", dname)
    case.launch()
    y, _ = case.results()
    u = UNIT[dtype]
    bound = u * want64.abs() + (1 + u) * 9 * c * 2.0 ** -24 * a + TINY[dtype]
    err = (y.double() - want64).abs()
    excess = float((err - u * want64.abs()).clamp_min(0).div(a.clamp_min(1e-300)).max())
    print(f"{shape} {dname}: max (|y - y64| - u |y64|)+ / A = {excess:.3e} (fp32 term of the bound {9 * c * 2.0 ** -24:.3e}), "
          f"max |y - y64| / max |y64| = {float(err.max() / want64.abs().max()):.3e}")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


def _bn_statistics(mom, n):
    """(save_mean, save_inv, running_mean, running_var) [n] float64 from mrla_bn_stats_fwd_rows on the records."""
    from mrla_amd import _lib as L, functional as Fm
    dev = "cuda"
    rec = mom.to(dev).contiguous()
    gamma, beta = torch.ones(n, device=dev), torch.zeros(n, device=dev)
    rm, rv = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    buf = torch.empty((4, n), device=dev)
    L.call("mrla_bn_stats_fwd_rows", rec.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), L.BN_TRAIN,
           0.1, 1e-5, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), rec.shape[0], n, Fm._stream())
    torch.cuda.synchronize()
    return buf[2].double().cpu(), buf[3].double().cpu(), rm.double().cpu(), rv.double().cpu()


@pytest.mark.parametrize("shape,kind,dname", [((2, 64, 128, 7, 7, 1), "normal", "bf16"), ((1, 128, 128, 14, 14, 2), "normal", "f16"),
                                              ((5, 64, 64, 28, 28, 1), "normal", "bf16"), ((1, 64, 64, 3, 131, 2), "normal", "bf16"),
                                              ((2, 512, 512, 7, 7, 1), "normal", "f16"), ((5, 64, 64, 28, 28, 1), "positive", "bf16"),
                                              ((3, 128, 64, 8, 33, 1), "positive", "bf16")],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_the_records_are_the_moments_of_the_stored_outputs(shape, kind, dname):
    b, c, n, h, w, s = shape
    case = _Case(shape, kind, dname)
    case.launch()
    y, mom = case.results()
    m = b * case.ho * case.wo
    assert bool(mom[:, :, 3].double().sum(0).eq(m).all())             # every pixel counted once per channel
    y64 = y.double().permute(0, 2, 3, 1).reshape(m, n)
    sums = raw_sums(mom)
    assert relmax(sums[:, 0].numpy(), y64.sum(0).numpy()) < 1e-5 and relmax(sums[:, 1].numpy(), (y64 * y64).sum(0).numpy()) < 1e-5
    # no records requested: the same y, bit for bit
    bare = _Case(shape, kind, dname, moments=False)
    bare.launch()
    y2, _ = bare.results()
    assert torch.equal(_bits(y2), _bits(y))
    # the BatchNorm statistics pass on the records: the batch statistics of the stored tensor (the bounds of
    # test_conv_bn_statistics_when_the_mean_dwarfs_sigma: the mean to 1e-5 of itself, the variance to 1e-4 of itself)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    if kind == "positive":
        ratio = float((mean.abs() / var.sqrt()).median())
        print(f"{shape}: |mean| / sigma = {ratio:.1f}")
        assert ratio >= 30.0 and bool((var > 1e3 * 1e-5).all())
    save_mean, save_inv, rm, rv = _bn_statistics(mom, n)
    scale = mean.abs() if kind == "positive" else mean.abs() + var.sqrt()      # (a mean near 0 is known to sigma, not to itself)
    e_mean = float(((save_mean - mean).abs() / scale).max())
    e_var = float(((1.0 / (save_inv * save_inv) - 1e-5 - var).abs() / var).max())
    print(f"{shape} {kind}: mean error {e_mean:.2e}, variance error {e_var:.2e}")
    assert e_mean < 1e-5 and e_var < 1e-4
    assert float(((rm - 0.1 * mean).abs() / (0.1 * scale)).max()) < 1e-5
    if m > 1:
        assert float(((rv - (0.9 + 0.1 * var * m / (m - 1))).abs() / (0.1 * var)).max()) < 1e-4


@pytest.mark.parametrize("shape", [(2, 64, 128, 7, 7, 1), (5, 64, 64, 28, 28, 1), (1, 128, 128, 14, 14, 2)], ids=_ids)
def test_two_calls_are_bit_equal_whatever_the_buffers_held(shape):
    case = _Case(shape, "normal", "bf16")
    case.launch()
    y0, mom0 = case.results()
    case.new_outputs()                                   # fresh NaN-patterned buffers at other addresses
    case.launch()
    y1, mom1 = case.results()
    case.gy.payload.fill_(-7.0)                          # ... and into buffers that held ordinary numbers
    case.gmom.payload.fill_(3.0)
    case.launch()
    torch.cuda.synchronize()
    y2, mom2 = case.gy.payload.cpu(), case.gmom.payload.cpu()
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(mom1), _bits(mom0))
    assert torch.equal(_bits(y2), _bits(_nhwc(y0)).reshape(-1)) and torch.equal(_bits(mom2), _bits(mom0).reshape(-1))


@pytest.mark.parametrize("shape", REPLAY_SHAPES, ids=_ids)
def test_replays_of_a_captured_call_are_bit_equal_to_the_eager_call(shape):
    case = _Case(shape, "normal", "bf16")
    case.launch()
    y0, mom0 = case.results()
    want64, a = _reference(shape, "normal", "bf16")
    assert float((y0.double() - want64).abs().max() / want64.abs().max()) < 2.0 ** -7      # (the eager call is the right answer)
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
        y, mom = case.results()
        assert torch.equal(_bits(y), _bits(y0)), f"replay {i}: y differs from the eager call"
        assert torch.equal(_bits(mom), _bits(mom0)), f"replay {i}: mom_part differs from the eager call"


# ---- the input gradient at stride 1: the same entry point on dy and the flipped, transposed weight ----------------------

@functools.lru_cache(maxsize=None)
def _dgrad_inputs(shape, kind, dname="bf16"):
    b, c, n, h, w, s = shape
    gen = torch.Generator().manual_seed(77 + 1000 * h + 10 * w + c + n + b + (0 if kind == "int" else 7))
    if kind == "int":
        dy = torch.randint(-4, 5, (b, n, h, w), generator=gen).double()
        wt = torch.randint(-2, 3, (n, c, 3, 3), generator=gen).double()
    else:
        dy = torch.randn((b, n, h, w), generator=gen).to(DTYPES[dname]).double()
        wt = (torch.randn((n, c, 3, 3), generator=gen) * (2.0 / (9 * n)) ** 0.5).to(DTYPES[dname]).double()
    return dy, wt


def _dx64(dy, wt, shape):
    b, c, n, h, w, s = shape
    x = torch.zeros((b, c, h, w), dtype=torch.float64)
    dx, _, _ = torch.ops.aten.convolution_backward(dy, x, wt, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, [True, False, False])
    return dx


@functools.lru_cache(maxsize=None)
def _dgrad_reference(shape, kind, dname="bf16"):
    dy, wt = _dgrad_inputs(shape, kind, dname)
    return _dx64(dy, wt, shape), _dx64(dy.abs(), wt.abs(), shape)


def _own_dx(shape, kind, dname):
    from mrla_amd import _lib as L, functional as Fm
    b, c, n, h, w, s = shape
    dtype = DTYPES[dname]
    dy, wt = _dgrad_inputs(shape, kind, dname)
    wflip = wt.flip(2, 3).transpose(0, 1)                                  # [c, n, 3, 3]: wflip[c, kh, kw, n] = wt[n, 2-kh, 2-kw, c]
    gdy = _Guarded(dy.numel(), h * w * n, dtype, _nhwc(dy))
    gw = _Guarded(wt.numel(), 9 * n, dtype, _nhwc(wflip))
    gdx = _Guarded(b * h * w * c, w * c, dtype)
    L.call("mrla_conv3x3_fwd", gdy.ptr(), gw.ptr(), gdx.ptr(), None, b, n, c, h, w, 1, Fm._DT[dtype], Fm._stream())
    torch.cuda.synchronize()
    return gdx.check_output("dx").view(b, h, w, c).permute(0, 3, 1, 2)


STRIDE1 = [s for s in SHAPES if s[5] == 1]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", STRIDE1, ids=_ids)
def test_the_input_gradient_at_stride_1_is_the_same_entry_point(shape, dname):
    b, c, n, h, w, s = shape
    dtype = DTYPES[dname]
    want64, a = _dgrad_reference(shape, "int")
    assert float(a.max()) < 2 ** 24
    dx = _own_dx(shape, "int", dname)
    bad = _bits(dx) != _bits((want64 + 0.0).float().to(dtype))
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
    want64, a = _dgrad_reference(shape, "normal", dname)
    dx = _own_dx(shape, "normal", dname)
    u = UNIT[dtype]
    bound = u * want64.abs() + (1 + u) * 9 * n * 2.0 ** -24 * a + TINY[dtype]
    err = (dx.double() - want64).abs()
    excess = float((err - u * want64.abs()).clamp_min(0).div(a.clamp_min(1e-300)).max())
    print(f"{shape} {dname}: dx max (|dx - dx64| - u |dx64|)+ / A = {excess:.3e} (fp32 term of the bound {9 * n * 2.0 ** -24:.3e})")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"
