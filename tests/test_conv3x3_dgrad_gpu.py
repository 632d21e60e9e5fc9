"""GPU: mrla_conv3x3_dgrad_s2 (mrla_amd/csrc/conv3x3_dgrad.hip) through the C ABI against float64 on the CPU --
aten.convolution_backward(dy64, x, wt64, stride 2, padding 1) masked to the input gradient.

1. Exact: integer-valued dy in [-4, 4] and wt in [-2, 2]: every fp32 partial sum is an integer below 4 * 512 * 8 < 2^24, exact
   in ANY order, so dx must equal the float64 gradient cast once to the dtype, bit for bit.  dx sits inside NaN-patterned
   guards (untouched afterwards, no payload element left unwritten), dy and wt inside guards of 2^14 (a read outside them
   breaks the equality).
2. Normal data rounded to the dtype first: |dx - dx64| <= u |dx64| + (1 + u) 4n 2^-24 A + t, A = the same gradient of |dy|,
   |wt| in float64 (any summation order of at most 4n terms in fp32 -- an odd-odd pixel meets four taps -- then ONE rounding
   of relative size u = 2^-8 bf16, 2^-11 fp16; t = half the smallest subnormal, where the format is a fixed grid).  Derived,
   not measured; the measured maximum is printed.
3. Determinism: further calls into fresh NaN-patterned buffers and into buffers that held ordinary numbers are bit-equal.
4. Replay: three replays of a captured call (dx overwritten with the NaN pattern in between) equal the eager call."""
import functools

import pytest
import torch

from tests.test_stem_exact_gpu import INT_OF, _Guarded, _bits, _nhwc

pytestmark = pytest.mark.gpu

SHAPES = [                       # (b, c, n, h, w)
    (1, 64, 64, 1, 1),           # one even pixel, one tap
    (1, 64, 64, 2, 1),
    (1, 64, 64, 2, 2),           # all four classes, one cell
    (1, 64, 64, 3, 5),           # odd by odd
    (2, 64, 128, 8, 8),          # even map, c != n, an image boundary below an odd row
    (2, 64, 64, 7, 7),
    (2, 128, 64, 9, 6),
    (1, 128, 128, 14, 14),
    (2, 256, 256, 14, 14),       # several n-chunks
    (2, 512, 512, 6, 6),         # eight chunks
    (5, 64, 64, 28, 28),         # several steps per workgroup, a range crossing images
    (1, 64, 64, 3, 131),         # rows wider than a segment, odd width
    (1, 64, 64, 2, 250),         # ... and even width
]
REPLAY_SHAPES = [(2, 512, 512, 6, 6), (1, 128, 128, 14, 14)]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}       # half the smallest subnormal
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _plan(shape, dt):
    from mrla_amd import _lib as L
    plan = L.conv3x3_dgrad_s2_plan(*shape, dt)
    assert plan is not None
    return plan


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, dname="bf16"):
    """float64 CPU tensors dy [b, n, ho, wo] and wt [n, c, 3, 3]: integers, or normal data rounded to the dtype."""
    b, c, n, h, w = shape
    ho, wo = _out_hw(h, w)
    gen = torch.Generator().manual_seed(2000 + 1000 * h + 10 * w + c + n + b + (0 if kind == "int" else 7))
    if kind == "int":
        dy = torch.randint(-4, 5, (b, n, ho, wo), generator=gen).double()
        wt = torch.randint(-2, 3, (n, c, 3, 3), generator=gen).double()
    else:
        dy = torch.randn((b, n, ho, wo), generator=gen).to(DTYPES[dname]).double()
        wt = (torch.randn((n, c, 3, 3), generator=gen) * (2.0 / (9 * n)) ** 0.5).to(DTYPES[dname]).double()
    return dy, wt


def _dx64(dy, wt, shape):
    b, c, n, h, w = shape
    x = torch.zeros((b, c, h, w), dtype=torch.float64)
    dx, _, _ = torch.ops.aten.convolution_backward(dy, x, wt, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1, [True, False, False])
    return dx


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dname="bf16"):
    """(dx64, A) [b, c, h, w]: the float64 input gradient and the same of |dy|, |wt|.  Computed once per case, never modified."""
    dy, wt = _inputs(shape, kind, dname)
    return _dx64(dy, wt, shape), _dx64(dy.abs(), wt.abs(), shape)


class _Case:
    """The guarded device buffers of one call, and the call."""

    def __init__(self, shape, kind, dname):
        from mrla_amd import functional as Fm
        self.shape, self.dtype = shape, DTYPES[dname]
        self.dt = Fm._DT[self.dtype]
        b, c, n, h, w = shape
        ho, wo = _out_hw(h, w)
        dy, wt = _inputs(shape, kind, dname)
        _plan(shape, self.dt)
        self.gdy = _Guarded(dy.numel(), ho * wo * n, self.dtype, _nhwc(dy))
        self.gw = _Guarded(wt.numel(), 9 * c, self.dtype, _nhwc(wt))          # [n, 3, 3, c]: the forward's own layout
        self.new_outputs()

    def new_outputs(self):
        b, c, n, h, w = self.shape
        self.gdx = _Guarded(b * h * w * c, w * c, self.dtype)

    def refill_outputs(self):
        self.gdx.flat.view(INT_OF[self.dtype]).fill_(self.gdx._pattern())

    def launch(self):
        from mrla_amd import _lib as L, functional as Fm
        L.call("mrla_conv3x3_dgrad_s2", self.gdy.ptr(), self.gw.ptr(), self.gdx.ptr(), *self.shape, self.dt, Fm._stream())

    def result(self):
        """dx [b, c, h, w] on the CPU, after the guard checks."""
        torch.cuda.synchronize()
        b, c, n, h, w = self.shape
        return self.gdx.check_output("dx").view(b, h, w, c).permute(0, 3, 1, 2)


def test_the_cases_cover_what_they_are_for():
    """Through the plan: a row cut into segments, several steps in a workgroup, a range of cell rows over two images, several
    n-chunks, several ranges, odd and even sizes in both directions."""
    from mrla_amd import _lib as L
    segments = steps = spans = chunks = ranges_ = False
    for shape in SHAPES:
        b, c, n, h, w = shape
        tc, per, rstep, nseg, ranges, wgs = _plan(shape, L.BF16)
        ho = _out_hw(h, w)[0]
        assert ranges == -(-b * ho // per) and wgs == ranges * (c // tc) and rstep >= 1 and nseg >= 1
        segments |= nseg > 1
        for i in range(ranges):
            lo, hi = i * per, min(b * ho, (i + 1) * per)
            nsteps, r = 0, lo
            while r < hi:                                  # steps of a range: cell rows of one image, at most rstep at a time
                r += min(rstep, ho - r % ho, hi - r)
                nsteps += 1
            steps |= nsteps > 1
            spans |= lo // ho != (hi - 1) // ho
        chunks |= n > 64
        ranges_ |= ranges > 1
    assert segments and steps and spans and chunks and ranges_
    assert {(s[3] % 2, s[4] % 2) for s in SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_integer_inputs_give_the_float64_gradient_bit_for_bit_inside_guards(shape, dname):
    want64, a = _reference(shape, "int")
    assert float(a.max()) < 2 ** 24 and torch.equal(want64.round(), want64)
    want = (want64 + 0.0).float().to(DTYPES[dname])
    case = _Case(shape, "int", dname)
    case.launch()
    dx = case.result()
    if shape == (1, 64, 64, 1, 1):
        dy, wt = _inputs(shape, "int")
        assert torch.equal(want64[0, :, 0, 0], dy[0, :, 0, 0] @ wt[:, :, 1, 1])
    bad = _bits(dx) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_normal_inputs_stay_inside_the_fp32_summation_bound(shape, dname):
    b, c, n, h, w = shape
    dtype = DTYPES[dname]
    want64, a = _reference(shape, "normal", dname)
    case = _Case(shape, "normal", dname)
    case.launch()
    dx = case.result()
    u = UNIT[dtype]
    bound = u * want64.abs() + (1 + u) * 4 * n * 2.0 ** -24 * a + TINY[dtype]
    err = (dx.double() - want64).abs()
    excess = float((err - u * want64.abs()).clamp_min(0).div(a.clamp_min(1e-300)).max())
    print(f"{shape} {dname}: max (|dx - dx64| - u |dx64|)+ / A = {excess:.3e} (fp32 term of the bound {4 * n * 2.0 ** -24:.3e}), "
          f"max |dx - dx64| / max |dx64| = {float(err.max() / want64.abs().max()):.3e}")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("shape", [(2, 64, 128, 8, 8), (5, 64, 64, 28, 28), (1, 64, 64, 3, 131)], ids=_ids)
def test_two_calls_are_bit_equal_whatever_the_buffers_held(shape):
    case = _Case(shape, "normal", "bf16")
    case.launch()
    dx0 = case.result()
    case.new_outputs()                                   # a fresh NaN-patterned buffer at another address
    case.launch()
    dx1 = case.result()
    case.gdx.payload.fill_(-7.0)                         # ... and into a buffer that held ordinary numbers
    case.launch()
    torch.cuda.synchronize()
    dx2 = case.gdx.payload.cpu()
    assert torch.equal(_bits(dx1), _bits(dx0))
    assert torch.equal(_bits(dx2), _bits(_nhwc(dx0)).reshape(-1))


@pytest.mark.parametrize("shape", REPLAY_SHAPES, ids=_ids)
def test_replays_of_a_captured_call_are_bit_equal_to_the_eager_call(shape):
    case = _Case(shape, "normal", "bf16")
    case.launch()
    dx0 = case.result()
    want64, a = _reference(shape, "normal", "bf16")
    assert float((dx0.double() - want64).abs().max() / want64.abs().max()) < 2.0 ** -7      # (the eager call is the right answer)
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
        dx = case.result()
        assert torch.equal(_bits(dx), _bits(dx0)), f"replay {i}: dx differs from the eager call"
