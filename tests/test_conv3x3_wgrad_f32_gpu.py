"""GPU: mrla_conv3x3_f32_wgrad (mrla_amd/csrc/conv3x3_wgrad_f32.hip) through the C ABI against float64 on the CPU -- autograd.grad
of F.conv2d(x64, w64, stride=s, padding=1) with respect to w64, permuted to the kernel's [n, 3, 3, c].  The shapes, the
reference and the guards are those of tests/test_conv3x3_wgrad_gpu.py; x, dy, part and dw are fp32.

1. Exact: inputs on dyadic grids (x in halves of -4..4, dy in quarters of -4..4), so every product is a multiple of 1/8 of
   magnitude <= 2 and every partial sum over the <= 2^17 pixels here is exact in fp32 in ANY order: dw must equal the float64
   gradient bit for bit.  dw and part sit inside NaN-patterned guards (untouched afterwards, no payload element left
   unwritten), x and dy inside guards of 2^14 (a read outside them breaks the equality).
2. Random data: fp32 normal inputs.  Any summation order of m fused products in fp32 has error at most m * 2^-24 * A, A being
   the same gradient of |x| and |dy|; the bound asserted is (m + 9) * 2^-24 * A elementwise, with no storage term (dw is
   fp32, the sums themselves).  Derived, not measured.
3. Determinism: a second call into freshly NaN-patterned part and dw, and a third into buffers that held ordinary numbers,
   are bit-equal in dw and part.
4. Replay: for the two 512-wide batch-8 shapes, three replays of a captured call (dw and part overwritten with the NaN
   pattern in between) are bit-equal to the eager call."""
import functools

import pytest
import torch

from tests.test_conv3x3_wgrad_gpu import REPLAY_SHAPES, SHAPES, _dw64, _ids, _out_hw
from tests.test_stem_exact_gpu import INT_OF, NAN_BITS, _Guarded, _bits, _nhwc

pytestmark = pytest.mark.gpu

assert len(SHAPES) == 14 and REPLAY_SHAPES == [(8, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2)]
assert NAN_BITS[torch.float32] >> 23 == 0xFF and INT_OF[torch.float32] == torch.int32       # (the pattern is a NaN of fp32)


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """float64 CPU tensors x [b, c, h, w], dy [b, n, ho, wo]: on the dyadic grids, or fp32 normal numbers."""
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    gen = torch.Generator().manual_seed(100000 * s + 1000 * h + 10 * w + c + n + b + (32 if kind == "dyadic" else 39))
    if kind == "dyadic":
        x = torch.randint(-4, 5, (b, c, h, w), generator=gen).double() / 2
        dy = torch.randint(-4, 5, (b, n, ho, wo), generator=gen).double() / 4
    else:
        x = torch.randn((b, c, h, w), generator=gen, dtype=torch.float32).double()
        dy = torch.randn((b, n, ho, wo), generator=gen, dtype=torch.float32).double()
    return x, dy


@functools.lru_cache(maxsize=None)
def _reference(shape, kind):
    """(dw64, A) [n, 3, 3, c]: the float64 gradient and the same gradient of |x|, |dy|.  Computed once per case, never modified."""
    x, dy = _inputs(shape, kind)
    return _dw64(x, dy, shape[5]), _dw64(x.abs(), dy.abs(), shape[5])


def _plan(shape):
    from mrla_amd import _lib as L
    plan = L.conv3x3_f32_wgrad_plan(*shape)
    rows = L.load().mrla_conv3x3_f32_wgrad_rows(*shape)
    assert plan is not None and rows == plan[4] > 0
    return plan


class _Case:
    """The guarded device buffers of one call, and the call."""

    def __init__(self, shape, kind):
        self.shape = shape
        b, c, n, h, w, s = shape
        x, dy = _inputs(shape, kind)
        self.rows = _plan(shape)[4]
        self.nel = n * 9 * c
        self.gx = _Guarded(x.numel(), h * w * c, torch.float32, _nhwc(x))
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
        L.call("mrla_conv3x3_f32_wgrad", self.gdy.ptr(), self.gx.ptr(), self.gpart.ptr(), self.gdw.ptr(), *self.shape, Fm._stream())

    def results(self):
        """(dw [n, 3, 3, c], part) on the CPU, after the guard checks."""
        torch.cuda.synchronize()
        b, c, n, h, w, s = self.shape
        dw = self.gdw.check_output("dw").view(n, 3, 3, c)
        part = self.gpart.check_output("part")
        return dw, part


def test_the_cases_cover_what_they_are_for():
    """Through the fp32 plan: a split boundary inside an image, >= 2 output tiles along each of n and c."""
    inside = tiles2 = False
    for shape in SHAPES:
        b, c, n, h, w, s = shape
        tn, tc, per, stages, splits, tiles = _plan(shape)
        ho = _out_hw(h, w, s)[0]
        assert splits == -(-b * ho // per) and tiles == (n // tn) * (c // tc) and stages >= 1
        inside |= splits >= 2 and any((i * per) % ho for i in range(1, splits))
        tiles2 |= n // tn >= 2 and c // tc >= 2
    assert inside and tiles2


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_inputs_give_the_float64_gradient_bit_for_bit_inside_guards(shape):
    want64, a = _reference(shape, "dyadic")
    # exactness of every fp32 partial sum, in any order: multiples of 1/8 bounded by the sum of the magnitudes
    assert float(a.max()) * 8 < 2 ** 24 and torch.equal((want64 * 8).round(), want64 * 8)
    want = (want64 + 0.0).float()                        # (+ 0.0: the accumulators start at +0, a sum of zeros is +0)
    assert torch.equal(want.double(), want64)
    case = _Case(shape, "dyadic")
    case.launch()
    dw, _ = case.results()
    if shape == (1, 64, 64, 1, 1, 1):
        off_centre = want64.clone()
        off_centre[:, 1, 1, :] = 0
        assert not bool(off_centre.any()) and bool(want64[:, 1, 1, :].any())
    bad = _bits(dw) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_inputs_stay_inside_the_fp32_summation_bound(shape):
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
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


@pytest.mark.parametrize("shape", [(1, 128, 128, 14, 14, 2), (5, 64, 64, 28, 28, 1), (2, 256, 256, 14, 14, 1)], ids=_ids)
def test_two_calls_are_bit_equal_whatever_the_buffers_held(shape):
    """One shape at stride 2, one with several splits, one with several tiles."""
    plans = {sh: _plan(sh) for sh in [(5, 64, 64, 28, 28, 1), (2, 256, 256, 14, 14, 1)]}
    assert plans[(5, 64, 64, 28, 28, 1)][4] >= 2 and plans[(2, 256, 256, 14, 14, 1)][5] >= 2
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


@pytest.mark.parametrize("shape", REPLAY_SHAPES, ids=_ids)
def test_replays_of_a_captured_call_are_bit_equal_to_the_eager_call(shape):
    case = _Case(shape, "normal")
    case.launch()
    dw0, part0 = case.results()
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
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
