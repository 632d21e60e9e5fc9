"""GPU: mrla_stem_conv_wgrad (mrla_amd/csrc/stem_wgrad.hip) through the C ABI against float64 on the CPU -- autograd.grad of
F.conv2d(x64, w64, stride=2, padding=3) with respect to w64, permuted to the kernel's [n, 7, 7, 3].

1. Exact: inputs on dyadic grids (x in halves of -4..4, dy in quarters of -4..4), so every product is a multiple of 1/8 of
   magnitude <= 2 and every partial sum over the < 2^17 pixels here is exact in fp32 in ANY order: dw must equal the float64
   gradient, rounded once to dw_dtype, bit for bit.  dw and part sit inside NaN-patterned guards (untouched afterwards, no
   payload element left unwritten), x and dy inside guards of 2^14 (a read outside them breaks the equality).
2. Random data: normal inputs rounded to the dtype first.  Any summation order of m terms in fp32 has error at most
   m * 2^-24 * A, A being the same gradient of |x| and |dy|; the bound asserted is (m + 9) * 2^-24 * A elementwise with
   m = b * ho * wo, plus u * |dw64| (u = 2^-8 bf16, 2^-11 fp16) where dw is stored in 16 bits -- and, for fp16 values below
   2^-14, where the format is a fixed grid of 2^-24, half that step (tests/test_conv3x3_wgrad_gpu.py).  Derived, not measured.
3. Determinism: a second call into freshly NaN-patterned part and dw is bit-equal -- the result does not depend on what the
   buffers held.
4. Replay: at the two smallest multi-split shapes, three replays of a captured call (dw and part overwritten with the NaN
   pattern in between) are bit-equal to the eager call.

The shapes are the smallest at which each mechanism can go wrong (see SHAPES); odd widths are served, so they are here."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_stem_exact_gpu import INT_OF, NAN_BITS, _Guarded, _bits, _nhwc  # noqa: F401

pytestmark = pytest.mark.gpu

SEGMENTS = "height 3, two column segments"      # (1, 64, 3, w): w from the plan, see _resolve
SHAPES = [                     # (b, n, h, w)
    (1, 64, 1, 1),             # only tap (3, 3) is non-zero, the other 48 exactly 0
    (1, 64, 2, 2),             # map smaller than the kernel
    (1, 64, 7, 8),             # every tap clipped somewhere
    (2, 64, 8, 8),             # image-to-image border
    (2, 64, 9, 6),             # odd height
    (1, 64, 5, 7),             # odd width (served: the 2-byte loads of x)
    (3, 128, 14, 10),          # two n tiles
    (5, 64, 40, 40),           # several splits with a ragged last one, a split boundary inside an image
    (2, 64, 64, 64),           # one plain multi-split shape
    SEGMENTS,                  # a row wider than one step: the first width with two column segments and a ragged last one
    (1, 64, 2, 258),           # ... (that width is odd) and on the 4-byte loads of an even width
]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
_ids = lambda s: s.replace(" ", "_").replace(",", "") if isinstance(s, str) else "x".join(map(str, s))  # noqa: E731


def _out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def _resolve(shape):
    """SEGMENTS -> (1, 64, 3, w) with w the first width whose plan has two column segments, the last one ragged."""
    if shape != SEGMENTS:
        return shape
    from mrla_amd import _lib as L
    for w in range(1, 4096):
        plan = L.stem_conv_wgrad_plan(1, 64, 3, w, L.BF16)
        if plan[3] == 2 and _out_hw(3, w)[1] % plan[5]:
            return (1, 64, 3, w)
    raise AssertionError("no width below 4096 needs two column segments")


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, dname="bf16"):
    """float64 CPU tensors x [b, 3, h, w], dy [b, n, ho, wo]: on the dyadic grids, or normal and rounded to the dtype."""
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + n + b + (0 if kind == "dyadic" else 7))
    if kind == "dyadic":
        x = torch.randint(-4, 5, (b, 3, h, w), generator=gen).double() / 2
        dy = torch.randint(-4, 5, (b, n, ho, wo), generator=gen).double() / 4
    else:
        x = torch.randn((b, 3, h, w), generator=gen).to(DTYPES[dname]).double()
        dy = torch.randn((b, n, ho, wo), generator=gen).to(DTYPES[dname]).double()
    return x, dy


def _dw64(x, dy):
    w = torch.zeros((dy.shape[1], 3, 7, 7), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=2, padding=3)
    assert y.shape == dy.shape
    (g,) = torch.autograd.grad(y, w, dy)
    return g.permute(0, 2, 3, 1).contiguous()            # [n, 7, 7, 3]


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dname="bf16"):
    """(dw64, A) [n, 7, 7, 3]: the float64 gradient and the same gradient of |x|, |dy|.  Computed once per case, never modified."""
    x, dy = _inputs(shape, kind, dname)
    return _dw64(x, dy), _dw64(x.abs(), dy.abs())


def _plan(shape, dt):
    from mrla_amd import _lib as L
    plan = L.stem_conv_wgrad_plan(*shape, dt)
    rows = L.load().mrla_stem_conv_wgrad_rows(*shape, dt)
    assert plan is not None and rows == plan[2] > 0
    return plan


class _Case:
    """The guarded device buffers of one call, and the call."""

    def __init__(self, shape, kind, dname, dw_dtype):
        from mrla_amd import functional as Fm
        self.shape, self.dtype, self.dw_dtype = shape, DTYPES[dname], dw_dtype
        self.dt, self.dwt = Fm._DT[self.dtype], Fm._DT[dw_dtype]
        b, n, h, w = shape
        x, dy = _inputs(shape, kind, dname)
        self.rows = _plan(shape, self.dt)[2]
        self.nel = n * 147
        self.gx = _Guarded(x.numel(), h * w * 3, self.dtype, _nhwc(x))
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
        L.call("mrla_stem_conv_wgrad", self.gdy.ptr(), self.gx.ptr(), self.gpart.ptr(), self.gdw.ptr(), *self.shape, self.dt,
               self.dwt, Fm._stream())

    def results(self):
        """(dw [n, 7, 7, 3], part) on the CPU, after the guard checks; inputs and their guards unchanged."""
        torch.cuda.synchronize()
        dw = self.gdw.check_output("dw").view(self.shape[1], 7, 7, 3)
        part = self.gpart.check_output("part")
        return dw, part


def _multi_split_shapes():
    """The shapes of SHAPES with more than one split, smallest input first."""
    from mrla_amd import _lib as L
    shapes = [_resolve(s) for s in SHAPES]
    return sorted((s for s in shapes if _plan(s, L.BF16)[2] >= 2), key=lambda s: (s[0] * s[2] * s[3], s))


def test_the_cases_cover_what_they_are_for():
    """Through the plan: a ragged last split and a split boundary inside an image at (5, 64, 40, 40), several splits at
    (2, 64, 64, 64), two n tiles, two column segments with a ragged last one, one split and many."""
    from mrla_amd import _lib as L
    tn, per, splits, nseg, lds, ws, rmax = _plan((5, 64, 40, 40), L.BF16)
    ho = 20
    assert splits >= 3 and (5 * ho) % per != 0 and splits == -(-5 * ho // per)          # ragged last split
    assert any((i * per) % ho for i in range(1, splits))                                # a boundary inside an image
    assert _plan((2, 64, 64, 64), L.BF16)[2] >= 2 and _plan((1, 64, 1, 1), L.BF16)[2] == 1
    assert 128 // _plan((3, 128, 14, 10), L.BF16)[0] == 2
    b, n, h, w = _resolve(SEGMENTS)
    tn, per, splits, nseg, lds, ws, rmax = _plan((b, n, h, w), L.BF16)
    assert h == 3 and nseg == 2 and 0 < _out_hw(h, w)[1] - ws < ws
    assert len(_multi_split_shapes()) >= 2


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_inputs_give_the_float64_gradient_bit_for_bit_inside_guards(shape, dname, wide):
    shape = _resolve(shape)
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    want64, a = _reference(shape, "dyadic")
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    # exactness of every fp32 partial sum, in any order: multiples of 1/8 bounded by the sum of the magnitudes
    assert b * ho * wo < 2 ** 17 and float(a.max()) * 8 < 2 ** 24 and torch.equal((want64 * 8).round(), want64 * 8)
    want = (want64 + 0.0).float().to(dw_dtype)           # (+ 0.0: the accumulators start at +0, a sum of zeros is +0)
    assert torch.equal(want64.float().double(), want64)
    case = _Case(shape, "dyadic", dname, dw_dtype)
    case.launch()
    dw, _ = case.results()
    if shape == (1, 64, 1, 1):
        off_centre = want64.clone()
        off_centre[:, 3, 3, :] = 0
        assert not bool(off_centre.any()) and bool(want64[:, 3, 3, :].any())
    bad = _bits(dw) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_inputs_stay_inside_the_fp32_summation_bound(shape, dname, wide):
    shape = _resolve(shape)
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    want64, a = _reference(shape, "normal", dname)
    case = _Case(shape, "normal", dname, dw_dtype)
    case.launch()
    dw, _ = case.results()
    m = b * ho * wo
    store = UNIT[dw_dtype] * want64.abs()
    if dw_dtype == torch.float16:
        # below 2^-14 fp16 is a fixed grid of 2^-24: half a step is what the ONE correct rounding costs there
        store = torch.where(want64.abs() < 2.0 ** -14, torch.full_like(store, 2.0 ** -25), store)
    bound = (m + 9) * 2.0 ** -24 * a + store
    err = (dw.double() - want64).abs()
    ratio = float((err / a.clamp_min(1e-300)).max())
    print(f"{shape} {dname} dw {dw_dtype}: max |dw - dw64| / A = {ratio:.3e} (fp32 term of the bound {(m + 9) * 2.0 ** -24:.3e})")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("shape", [(2, 64, 9, 6), (3, 128, 14, 10), (5, 64, 40, 40)], ids=_ids)
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


@pytest.mark.parametrize("which", [0, 1], ids=["smallest", "second_smallest"])
def test_replays_of_a_captured_call_are_bit_equal_to_the_eager_call(which):
    shape = _multi_split_shapes()[which]
    case = _Case(shape, "normal", "bf16", torch.float32)
    assert case.rows >= 2
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
