"""GPU: the one-step-ahead loader of mrla_conv3x3_wgrad (mrla_amd/csrc/conv3x3_wgrad.hip) at shapes where ONE workgroup walks
several steps of DIFFERENT geometry -- what a loader that fetches step i + 1 under the products of step i can get wrong (the
pieces of the wrong step in the raster, a stale predicate, a prefetch behind the last step), and what the shapes of
tests/test_conv3x3_wgrad_gpu.py, mostly one step per workgroup, do not reach.  By the planner's arithmetic (64 x 64 tiles, two
workgroups per CU; a step holds whole rows of ONE image, at most 128 raster pixels at stride 1 and 96 at stride 2, the raster
pitch at most 60):

  * (18, 512, 512, 4, 5, 1) and (18, 512, 512, 8, 9, 2): 64 tiles, 8 splits of 9 of the 72 output rows, 4 rows an image: the
    steps of the first three ranges are R = 4, 4, 1 / 3, 4, 2 / 2, 4, 3 rows, image borders inside a range;
  * (4, 512, 512, 4, 70, 1) and (4, 512, 512, 5, 131, 2): two column segments per row, 58 / 59 and then 12 / 7 columns wide,
    several rows (= twice as many steps) per workgroup;
  * (5, 512, 512, 9, 7, 1): 45 rows in 8 splits of 6 -- ranges of one step and of two steps side by side.

Method of tests/test_conv3x3_wgrad_gpu.py, whose helpers this file uses; the reference is float64 autograd on the CPU, never
the kernel.  Dyadic inputs: every partial sum is exact in fp32 in any order, so dw must equal the float64 gradient, rounded
once to dw_dtype, bit for bit; dw and part are NaN-patterned before the call, free of the pattern afterwards, their guard rows
untouched.  A second call into dirty buffers is bit-equal, and so are three replays of one captured call."""
import pytest
import torch

from tests.test_conv3x3_wgrad_gpu import DTYPES, _Case, _bits, _ids, _out_hw, _plan, _reference

pytestmark = pytest.mark.gpu

SHAPES = [                       # (b, c, n, h, w, s)
    (18, 512, 512, 4, 5, 1),
    (18, 512, 512, 8, 9, 2),
    (4, 512, 512, 4, 70, 1),
    (4, 512, 512, 5, 131, 2),
    (5, 512, 512, 9, 7, 1),
]
MAX_KP = {1: 128, 2: 96}         # raster pixels of a step (conv3x3_wgrad.hip: kC3MaxKP1, kC3MaxKP2)
MAX_PY = 60                      # raster pitch (kC3MaxPY)


def _steps(shape, dt):
    """Per split, the list of (rows, columns) of its steps, from the plan's rows per split and the raster rule above."""
    b, c, n, h, w, s = shape
    ho, wo = _out_hw(h, w, s)
    per, splits = _plan(shape, dt)[2], _plan(shape, dt)[4]
    pad = 2 if s == 1 else 1
    if wo + pad <= MAX_PY:
        rmax, segs = max(1, min(ho, MAX_KP[s] // (wo + pad))), [wo]
    else:
        ws = MAX_PY - pad
        rmax, segs = 1, [min(ws, wo - x0) for x0 in range(0, wo, ws)]
    out = []
    for i in range(splits):
        r, end, steps = i * per, min(b * ho, (i + 1) * per), []
        while r < end:
            rr = min(rmax, ho - r % ho, end - r)
            steps += [(rr, cols) for cols in segs]
            r += rr
        out.append(steps)
    return out


def test_the_shapes_give_one_workgroup_steps_of_different_geometry():
    from mrla_amd import _lib as L
    for shape in SHAPES:
        assert _plan(shape, L.BF16)[5] == 64, shape                                       # 64 output tiles
    for shape in SHAPES[:4]:
        assert any(len(set(st)) >= 2 for st in _steps(shape, L.BF16)), shape              # some range: two kinds of step
    for shape in SHAPES[:2]:
        plan, steps = _plan(shape, L.BF16), _steps(shape, L.BF16)
        assert plan[2] == 9 and plan[4] == 8
        assert [[r for r, _ in st] for st in steps[:3]] == [[4, 4, 1], [3, 4, 2], [2, 4, 3]]
    assert _steps(SHAPES[2], L.BF16)[0][:2] == [(1, 58), (1, 12)] and len(_steps(SHAPES[2], L.BF16)[0]) >= 4
    assert _steps(SHAPES[3], L.BF16)[0][:2] == [(1, 59), (1, 7)] and len(_steps(SHAPES[3], L.BF16)[0]) >= 4
    lens = {len(st) for st in _steps(SHAPES[4], L.BF16)}
    assert _plan(SHAPES[4], L.BF16)[2] == 6 and lens == {1, 2}


@pytest.mark.parametrize("wide", [True, False], ids=["dw_f32", "dw_16"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dyadic_gradient_is_exact_and_dirty_buffers_and_replays_change_nothing(shape, dname, wide):
    dw_dtype = torch.float32 if wide else DTYPES[dname]
    want64, a = _reference(shape, "dyadic")
    assert float(a.max()) * 8 < 2 ** 24 and torch.equal((want64 * 8).round(), want64 * 8)      # every fp32 partial sum is exact
    want = (want64 + 0.0).float().to(dw_dtype)
    case = _Case(shape, "dyadic", dname, dw_dtype)
    case.launch()
    dw0, part0 = case.results()                              # (NaN-pattern-free payloads, untouched guards: _Guarded.check_output)
    bad = _bits(dw0) != _bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
    # the partial tiles sum to the gradient exactly, whatever the split
    assert torch.equal(part0.double().view(case.rows, -1).sum(0), want64.reshape(-1))

    case.gpart.payload.fill_(3.0)                            # a second call into buffers that held ordinary numbers
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
        assert torch.equal(_bits(dw), _bits(dw0)), f"replay {i}: dw differs from the eager call"
        assert torch.equal(_bits(part), _bits(part0)), f"replay {i}: part differs from the eager call"
