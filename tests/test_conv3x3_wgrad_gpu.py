"""GPU: mrla_conv3x3_wgrad (mrla_amd/csrc/conv3x3_wgrad.hip) through the C ABI against float64 on the CPU -- autograd.grad of
F.conv2d(x64, w64, stride=s, padding=1) with respect to w64, permuted to the kernel's [n, 3, 3, c].

1. Exact: inputs on dyadic grids (x in halves of -4..4, dy in quarters of -4..4), so every product is a multiple of 1/8 of
   magnitude <= 2 and every partial sum over the <= 2^17 pixels here is exact in fp32 in ANY order: dw must equal the float64
   gradient, rounded once to dw_dtype, bit for bit.  dw and part sit inside NaN-patterned guards (untouched afterwards, no
   payload element left unwritten), x and dy inside guards of 2^14 (a read outside them breaks the equality).
2. Random data: normal inputs rounded to the dtype first.  Any summation order of m terms in fp32 has error at most
   m * 2^-24 * A, A being the same gradient of |x| and |dy|; the bound asserted is (m + 9) * 2^-24 * A elementwise, plus
   u * |dw64| (u = 2^-8 bf16, 2^-11 fp16) where dw is stored in 16 bits -- and, for fp16 values below 2^-14, where the format
   is a fixed grid of 2^-24 and u * |dw64| is below what any stored number can meet, half that step.  Derived, not measured.
3. Determinism: a second call into freshly NaN-patterned part and dw is bit-equal -- the result does not depend on what the
   buffers held.
4. Replay: for the two 512-wide batch-8 shapes at which the stock library's split-K solver goes wrong from the second replay
   of a captured graph, three replays (dw and part overwritten with the NaN pattern in between) are bit-equal to the eager call.

The shapes are the smallest at which each mechanism can go wrong (see SHAPES)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_stem_exact_gpu import INT_OF, NAN_BITS, _Guarded, _bits, _nhwc

pytestmark = pytest.mark.gpu

SHAPES = [                       # (b, c, n, h, w, s)
    (1, 64, 64, 1, 1, 1),        # only the centre tap is non-zero, the other eight exactly 0
    (1, 64, 64, 2, 1, 2),        # map smaller than the kernel, stride 2
    (1, 64, 64, 3, 5, 1),        # small map
    (2, 64, 128, 7, 7, 1),       # n != c, image-to-image border
    (3, 128, 64, 8, 33, 1),      # a row longer than a 32-pixel chunk
    (2, 64, 64, 7, 7, 2),        # stride 2, odd both ways
    (2, 64, 64, 9, 6, 2),        # stride 2, odd height, even width
    (1, 128, 128, 14, 14, 2),    # stride 2, wider tile
    (2, 256, 256, 14, 14, 1),    # several output tiles
    (5, 64, 64, 28, 28, 1),      # several splits
    (8, 512, 512, 7, 7, 1),      # a shape the stock solver gets wrong under replay
    (8, 512, 512, 14, 14, 2),    # a shape the stock solver gets wrong under replay
    (1, 64, 64, 2, 70, 1),       # a row wider than one step's raster: column segments, stride 1
    (1, 64, 64, 3, 131, 2),      # ... stride 2, ragged last segment
]
REPLAY_SHAPES = [(8, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2)]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, dname="bf16"):
    """float64 CPU tensors x [b, c, h, w], dy [b, n, ho, wo]: on the dyadic grids, or normal and rounded to the dtype."""
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    gen = torch.Generator().manual_seed(100000 * s + 1000 * h + 10 * w + c + n + b + (0 if kind == "dyadic" else 7))
    if kind == "dyadic":
        x = torch.randint(-4, 5, (b, c, h, w), generator=gen).double() / 2
        dy = torch.randint(-4, 5, (b, n, ho, wo), generator=gen).double() / 4
    else:
        x = torch.randn((b, c, h, w), generator=gen).to(DTYPES[dname]).double()
        dy = torch.randn((b, n, ho, wo), generator=gen).to(DTYPES[dname]).double()
    return x, dy


def _dw64(x, dy, s):
    n, c = dy.shape[1], x.shape[1]
    w = torch.zeros((n, c, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=s, padding=1)
    assert y.shape == dy.shape
    (g,) = torch.autograd.grad(y, w, dy)
    return g.permute(0, 2, 3, 1).contiguous()            # [n, 3, 3, c]


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dname="bf16"):
    """(dw64, A) [n, 3, 3, c]: the float64 gradient and the same gradient of |x|, |dy|.  Computed once per case, never modified."""
    x, dy = _inputs(shape, kind, dname)
    return _dw64(x, dy, shape[5]), _dw64(x.abs(), dy.abs(), shape[5])


def _plan(shape, dt):
    from mrla_amd import _lib as L
    b, c, n, h, w, s = shape
    plan = L.conv3x3_wgrad_plan(b, c, n, h, w, s, dt)
    rows = L.load().mrla_conv3x3_wgrad_rows(b, c, n, h, w, s, dt)
    assert plan is not None and rows == plan[4] > 0
    return plan


class _Case:
    """The guarded device buffers of one call, and the call."""

    def __init__(self, shape, kind, dname, dw_dtype):
        from mrla_amd import functional as Fm
        self.shape, self.dtype, self.dw_dtype = shape, DTYPES[dname], dw_dtype
        self.dt, self.dwt = Fm._DT[self.dtype], Fm._DT[dw_dtype]
        b, c, n, h, w, s = shape
        x, dy = _inputs(shape, kind, dname)
        self.rows = _plan(shape, self.dt)[4]
        self.nel = n * 9 * c
        self.gx = _Guarded(x.numel(), h * w * c, self.dtype, _nhwc(x))
        self.gdy = _Guarded(dy.numel(), dy[0].numel(), self.dtype, _nhwc(dy))
        self.new_outputs()

    def new_outputs(self):
        self.gdw = _Guarded(self.nel, self.nel, self.dw_dtype)
        self.gpart = _Guarded(self.rows * self.nel, self.nel, torch.float32)

    def refill_outputs(self):
        for g in (self.gdw, self.gpart):
            g.flat.view(INT_OF[g.dtype]).fill_(g._pattern())

    def launch(self):
        from mrla_amd import _lib as L, functional as Fm
        b, c, n, h, w, s = self.shape
        L.call("mrla_conv3x3_wgrad", self.gdy.ptr(), self.gx.ptr(), self.gpart.ptr(), self.gdw.ptr(), b, c, n, h, w, s, self.dt,
               self.dwt, Fm._stream())

    def results(self):
        """(dw [n, 3, 3, c], part) on the CPU, after the guard checks; inputs and their guards unchanged."""
        torch.cuda.synchronize()
        b, c, n, h, w, s = self.shape
        dw = self.gdw.check_output("dw").view(n, 3, 3, c)
        part = self.gpart.check_output("part")
        return dw, part


def test_the_cases_cover_what_they_are_for():
    """Through the plan: a split boundary inside an image, >= 2 output tiles along each of n and c, one split and many."""
    from mrla_amd import _lib as L
    inside = tiles2 = False
    for shape in SHAPES:
        b, c, n, h, w, s = shape
        tn, tc, per, stages, splits, tiles = _plan(shape, L.BF16)
        ho = _out_hw(h, w, s)[0]
        assert splits == -(-b * ho // per) and tiles == (n // tn) * (c // tc) and stages >= 1
        inside |= splits >= 2 and any((i * per) % ho for i in range(1, splits))
        tiles2 |= n // tn >= 2 and c // tc >= 2
    assert inside and tiles2


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_inputs_give_the_float64_gradient_bit_for_bit_inside_guards(shape, dname, wide):
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    want64, a = _reference(shape, "dyadic")
    # exactness of every fp32 partial sum, in any order: multiples of 1/8 bounded by the sum of the magnitudes
    assert float(a.max()) * 8 < 2 ** 24 and torch.equal((want64 * 8).round(), want64 * 8)
    want = (want64 + 0.0).float().to(dw_dtype)           # (+ 0.0: the accumulators start at +0, a sum of zeros is +0)
    assert torch.equal(want64.float().double(), want64)
    case = _Case(shape, "dyadic", dname, dw_dtype)
    case.launch()
    dw, _ = case.results()
    if shape == (1, 64, 64, 1, 1, 1):
        off_centre = want64.clone()
        off_centre[:, 1, 1, :] = 0
        assert not bool(off_centre.any()) and bool(want64[:, 1, 1, :].any())
    bad = _bits(dw) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_inputs_stay_inside_the_fp32_summation_bound(shape, dname, wide):
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    want64, a = _reference(shape, "normal", dname)
    case = _Case(shape, "normal", dname, dw_dtype)
    case.launch()
    dw, _ = case.results()
    m = b * ho * wo
    store = UNIT[dw_dtype] * want64.abs()
    if dw_dtype == torch.float16:
        # below 2^-14 fp16 is a fixed grid of 2^-24: half a step is what the ONE correct rounding costs there, and u * |dw64|
        # is less than that -- a bound no stored fp16 number could meet (it shows at m = 1, where dw is one small product)
        store = torch.where(want64.abs() < 2.0 ** -14, torch.full_like(store, 2.0 ** -25), store)
    bound = (m + 9) * 2.0 ** -24 * a + store
    err = (dw.double() - want64).abs()
    ratio = float((err / a.clamp_min(1e-300)).max())
    print(f"{shape} {dname} dw {dw_dtype}: max |dw - dw64| / A = {ratio:.3e} (fp32 term of the bound {(m + 9) * 2.0 ** -24:.3e})")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("shape", [(2, 64, 128, 7, 7, 1), (5, 64, 64, 28, 28, 1), (1, 128, 128, 14, 14, 2)], ids=_ids)
def test_two_calls_are_bit_equal_whatever_the_buffers_held(shape):
    case = _Case(shape, "normal", "bf16", torch.float32)
    case.launch()
    dw0, part0 = case.results()
    case.new_outputs()                                   # fresh NaN-patterned buffers at other addresses
    case.launch()
    dw1, part1 = case.results()
    case.gpart.payload.fill_(3.0)                        # ... and into buffers that held ordinary numbers
    case.gdw.payload.fill_(-7.0)
    case.launch()
    torch.cuda.synchronize()
    dw2, part2 = case.gdw.payload.cpu().view_as(dw0), case.gpart.payload.cpu()
    for dw, part in ((dw1, part1), (dw2, part2)):
        assert torch.equal(_bits(dw), _bits(dw0)) and torch.equal(_bits(part), _bits(part0))


@pytest.mark.parametrize("shape", REPLAY_SHAPES, ids=_ids)
def test_replays_of_a_captured_call_are_bit_equal_to_the_eager_call(shape):
    case = _Case(shape, "normal", "bf16", torch.float32)
    case.launch()
    dw0, part0 = case.results()
    want64, a = _reference(shape, "normal", "bf16")
    assert float(((dw0.double() - want64).abs() / a.clamp_min(1e-300)).max()) < 1e-3      # (the eager call is the right answer)
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
        assert torch.equal(_bits(dw), _bits(dw0)), f"replay {i}: dw differs from the eager call"
        assert torch.equal(_bits(part), _bits(part0)), f"replay {i}: part differs from the eager call"
