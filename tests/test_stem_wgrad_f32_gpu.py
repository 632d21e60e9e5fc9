"""GPU: mrla_stem_conv_f32_wgrad (mrla_amd/csrc/stem_wgrad_f32.hip) through the C ABI against float64 on the CPU -- autograd.grad
of F.conv2d(x64, w64, stride=2, padding=3) with respect to w64, permuted to the kernel's [n, 7, 7, 3].  The shapes, the
reference and the guards are those of tests/test_stem_wgrad_gpu.py; x, dy, part and dw are fp32.

1. Exact: inputs on dyadic grids (x in halves of -4..4, dy in quarters of -4..4), so every product is a multiple of 1/8 of
   magnitude <= 2 and every partial sum over the m <= 2048 pixels here is a multiple of 1/8 below 2^21: exact in fp32 in ANY
   order, so dw must equal the float64 gradient bit for bit.  dw and part sit inside NaN-patterned guards (untouched
   afterwards, no payload element left unwritten), x and dy inside guards of 2^14 (a read outside them breaks the equality).
2. Random data: fp32 normal inputs.  Any summation order of m fused products in fp32 has error at most m * 2^-24 * A, A being
   the same gradient of |x| and |dy|; the bound asserted is (m + 9) * 2^-24 * A elementwise with m = b * ho * wo -- the derived
   bound of tests/test_stem_wgrad_gpu.py with no storage term (dw is fp32, the sums themselves).  Derived, not measured.
3. Determinism: a second call into freshly NaN-patterned part and dw, and a third into buffers that held ordinary numbers,
   are bit-equal in dw and part.
4. Replay: at the two smallest multi-split shapes, three replays of a captured call (dw and part overwritten with the NaN
   pattern in between) are bit-equal to the eager call.

The column-segment shape is found through the fp32 plan (its step differs from the 16-bit kernel's)."""
import functools

import pytest
import torch

from tests.test_stem_exact_gpu import INT_OF, NAN_BITS, _Guarded, _bits, _nhwc
from tests.test_stem_wgrad_gpu import SEGMENTS, SHAPES, _dw64, _ids, _out_hw

pytestmark = pytest.mark.gpu

assert SHAPES == [(1, 64, 1, 1), (1, 64, 2, 2), (1, 64, 7, 8), (2, 64, 8, 8), (2, 64, 9, 6), (1, 64, 5, 7), (3, 128, 14, 10),
                  (5, 64, 40, 40), (2, 64, 64, 64), SEGMENTS, (1, 64, 2, 258)]
assert NAN_BITS[torch.float32] >> 23 == 0xFF and INT_OF[torch.float32] == torch.int32       # (the pattern is a NaN of fp32)


@functools.lru_cache(maxsize=None)
def _resolve(shape):
    """SEGMENTS -> (1, 64, 3, w) with w the first width whose fp32 plan has two column segments, the last one ragged."""
    if shape != SEGMENTS:
        return shape
    from mrla_amd import _lib as L
    for w in range(1, 4096):
        plan = L.stem_conv_f32_wgrad_plan(1, 64, 3, w)
        if plan[3] == 2 and _out_hw(3, w)[1] % plan[5]:
            return (1, 64, 3, w)
    raise AssertionError("no width below 4096 needs two column segments")


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """float64 CPU tensors x [b, 3, h, w], dy [b, n, ho, wo]: on the dyadic grids, or fp32 normal numbers."""
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + n + b + (32 if kind == "dyadic" else 39))
    if kind == "dyadic":
        x = torch.randint(-4, 5, (b, 3, h, w), generator=gen).double() / 2
        dy = torch.randint(-4, 5, (b, n, ho, wo), generator=gen).double() / 4
    else:
        x = torch.randn((b, 3, h, w), generator=gen, dtype=torch.float32).double()
        dy = torch.randn((b, n, ho, wo), generator=gen, dtype=torch.float32).double()
    return x, dy


@functools.lru_cache(maxsize=None)
def _reference(shape, kind):
    """(dw64, A) [n, 7, 7, 3]: the float64 gradient and the same gradient of |x|, |dy|.  Computed once per case, never modified."""
    x, dy = _inputs(shape, kind)
    return _dw64(x, dy), _dw64(x.abs(), dy.abs())


def _plan(shape):
    from mrla_amd import _lib as L
    plan = L.stem_conv_f32_wgrad_plan(*shape)
    rows = L.load().mrla_stem_conv_f32_wgrad_rows(*shape)
    assert plan is not None and rows == plan[2] > 0
    return plan


class _Case:
    """The guarded device buffers of one call, and the call."""

    def __init__(self, shape, kind):
        self.shape = shape
        b, n, h, w = shape
        x, dy = _inputs(shape, kind)
        self.rows = _plan(shape)[2]
        self.nel = n * 147
        self.gx = _Guarded(x.numel(), h * w * 3, torch.float32, _nhwc(x))
        self.gdy = _Guarded(dy.numel(), dy[0].numel(), torch.float32, _nhwc(dy))
        self.new_outputs()

    def new_outputs(self):
        self.gdw = _Guarded(self.nel, self.nel, torch.float32)
        self.gpart = _Guarded(self.rows * self.nel, self.nel, torch.float32)

    def refill_outputs(self):
        for g in (self.gdw, self.gpart):
            g.flat.view(INT_OF[g.dtype]).fill_(g._pattern())

    def launch(self):
        from mrla_amd import _lib as L, functional as Fm
        L.call("mrla_stem_conv_f32_wgrad", self.gdy.ptr(), self.gx.ptr(), self.gpart.ptr(), self.gdw.ptr(), *self.shape, Fm._stream())

    def results(self):
        """(dw [n, 7, 7, 3], part) on the CPU, after the guard checks."""
        torch.cuda.synchronize()
        dw = self.gdw.check_output("dw").view(self.shape[1], 7, 7, 3)
        part = self.gpart.check_output("part")
        return dw, part


def _multi_split_shapes():
    """The shapes of SHAPES with more than one split, smallest input first."""
    shapes = [_resolve(s) for s in SHAPES]
    return sorted((s for s in shapes if _plan(s)[2] >= 2), key=lambda s: (s[0] * s[2] * s[3], s))


def test_the_cases_cover_what_they_are_for():
    """Through the fp32 plan: a ragged last split and a split boundary inside an image at (5, 64, 40, 40), several splits at
    (2, 64, 64, 64), two n tiles, two column segments with a ragged last one, an odd width, one split and many."""
    tn, per, splits, nseg, lds, ws, rmax = _plan((5, 64, 40, 40))
    ho = 20
    assert splits >= 3 and (5 * ho) % per != 0 and splits == -(-5 * ho // per)          # ragged last split
    assert any((i * per) % ho for i in range(1, splits))                                # a boundary inside an image
    assert _plan((2, 64, 64, 64))[2] >= 2 and _plan((1, 64, 1, 1))[2] == 1
    assert 128 // _plan((3, 128, 14, 10))[0] == 2
    b, n, h, w = _resolve(SEGMENTS)
    tn, per, splits, nseg, lds, ws, rmax = _plan((b, n, h, w))
    assert h == 3 and nseg == 2 and 0 < _out_hw(h, w)[1] - ws < ws
    assert any(_resolve(s)[3] % 2 for s in SHAPES) and any(_resolve(s)[2] % 2 for s in SHAPES)      # odd widths, odd heights
    assert _plan((1, 64, 2, 258))[3] == 2                                               # ... and segments at an even width
    assert len(_multi_split_shapes()) >= 2
    assert max(s[0] * _out_hw(s[2], s[3])[0] * _out_hw(s[2], s[3])[1] for s in map(_resolve, SHAPES)) <= 2048


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_inputs_give_the_float64_gradient_bit_for_bit_inside_guards(shape):
    shape = _resolve(shape)
    want64, a = _reference(shape, "dyadic")
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    # exactness of every fp32 partial sum, in any order: multiples of 1/8 bounded by the sum of the magnitudes, below 2^21
    assert b * ho * wo <= 2048 and float(a.max()) < 2 ** 21 and torch.equal((want64 * 8).round(), want64 * 8)
    want = (want64 + 0.0).float()                        # (+ 0.0: the accumulators start at +0, a sum of zeros is +0)
    assert torch.equal(want.double(), want64)
    case = _Case(shape, "dyadic")
    case.launch()
    dw, _ = case.results()
    if shape == (1, 64, 1, 1):
        off_centre = want64.clone()
        off_centre[:, 3, 3, :] = 0
        assert not bool(off_centre.any()) and bool(want64[:, 3, 3, :].any())
    bad = _bits(dw) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_inputs_stay_inside_the_fp32_summation_bound(shape):
    shape = _resolve(shape)
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    want64, a = _reference(shape, "normal")
    case = _Case(shape, "normal")
    case.launch()
    dw, _ = case.results()
    m = b * ho * wo
    bound = (m + 9) * 2.0 ** -24 * a
    err = (dw.double() - want64).abs()
    ratio = float((err / a.clamp_min(1e-300)).max())
    print(f"{shape} f32: max |dw - dw64| / A = {ratio:.3e} (the bound {(m + 9) * 2.0 ** -24:.3e})")
    assert bool((err <= bound).all()), f"worst excess {float((err - bound).max()):.3e}"


@pytest.mark.parametrize("shape", [(2, 64, 9, 6), (3, 128, 14, 10), (5, 64, 40, 40)], ids=_ids)
def test_two_calls_are_bit_equal_whatever_the_buffers_held(shape):
    case = _Case(shape, "normal")
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
    case = _Case(shape, "normal")
    assert case.rows >= 2
    case.launch()
    dw0, part0 = case.results()
    b, n, h, w = shape
    ho, wo = _out_hw(h, w)
    want64, a = _reference(shape, "normal")
    assert bool(((dw0.double() - want64).abs() <= (b * ho * wo + 9) * 2.0 ** -24 * a).all())     # (the eager call is the right answer)
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
