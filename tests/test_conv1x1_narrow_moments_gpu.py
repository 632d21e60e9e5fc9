"""The narrow 1x1-convolution GEMM (n = 64 / 128: conv1 of the bottlenecks, mrla_amd/csrc/conv1x1.hip) with its
BatchNorm-moment epilogue, on the shapes tests/test_conv1x1_steady_gpu.py leaves out -- that file has ONE narrow shape,
(56, 56, 256, 64).

The epilogue takes the moments on the lanes that store the output lines: a lane owns 8 consecutive channels over 4 pixel
rows of every 32-pixel block, the pivot is tile pixel 0 of the wave's first block, lanes that share channels are summed at
the end of the kernel.  So this file covers what depends on that mapping: two waves along n (n = 128), every k the kernel
is instantiated for (64 / 128 / 256, four- and eight-wave workgroups), ragged last blocks, and workgroups in which some
pixel-waves never get a block and must publish a record the merge skips.

Same checks and bounds as test_forward_gemm_and_moment_partials_in_steady_state: float64 product of the same bf16 operands
rounded once (<= 1 bf16 ulp); two launches bit-equal for Y and the records; the epilogue on / off stores the same Y;
counts sum to m; raw sums, mean (relative to sigma) and variance within 1e-5 of the float64 statistics of the stored
tensor, merged the way the per-channel kernel merges them.  Added: every record's pivot is a value Y holds in that channel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (h, w, k, n): the stage-2 entry's conv1 (two waves along n), the stage-1 entry's conv1, stage-2 conv1-like shapes
SHAPES = [(56, 56, 256, 128), (56, 56, 64, 64), (28, 28, 128, 128), (28, 28, 128, 64)]


def _ragged_m(m0, k, n):
    """The largest m < m0 with m % 32 != 0 that the planner takes with the double buffer refilled (as at m0)."""
    from mrla_amd import _lib as L
    for m in range(m0 - 1, m0 - 4000, -1):
        if m % 32 == 0:
            continue
        plan = L.conv1x1_plan(m, k, n)
        if plan is not None and plan[0] > plan[1]:
            return m
    raise AssertionError("no ragged pixel count near " + str(m0))


def _check(m, k, n, seed):
    from mrla_amd import _lib as L
    from tests.test_conv1x1_gpu import raw_sums
    from tests.test_conv1x1_steady_gpu import _assert_bf16_close, _operands, _run_fwd
    rows = L.conv1x1_plan(m, k, n)[3]
    assert rows == L.load().mrla_conv1x1_rows(m, k, n, L.BF16) and m % rows == 0
    x, w = _operands(m, k, n, seed=seed)
    y, part = _run_fwd(x, w, m, k, n, rows, True)
    y2, part2 = _run_fwd(x, w, m, k, n, rows, True)
    y3, _ = _run_fwd(x, w, m, k, n, rows, False)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs of the same launch differ"
    assert torch.equal(y, y3), "the kernel without the moments epilogue stores different outputs"
    want = x.double() @ w.double().t()
    _assert_bf16_close(y, want, "y")
    del want
    # counts: whole numbers, a record without pixels is all zero, together they are the tensor
    cnt = part[:, :, 3]
    assert torch.equal(cnt, cnt.round()) and (cnt >= 0).all()
    assert cnt.double().sum(0).eq(m).all()
    assert (part[cnt == 0] == 0).all(), "a record without pixels is not empty"
    # every pivot is an output of its channel
    yf = y.float()
    for c in range(n):
        used = part[:, c, 3] > 0
        assert torch.isin(part[used, c, 2], yf[:, c]).all(), f"channel {c}: a pivot that is not one of its outputs"
    # statistics of the stored (rounded) tensor
    g = y.double()
    s = raw_sums(part)
    s1, s2 = g.sum(0), (g * g).sum(0)
    e1 = ((s[:, 0] - s1).abs().max() / s1.abs().max()).item()
    e2 = ((s[:, 1] - s2).abs().max() / s2.abs().max()).item()
    # ... and the mean / variance the per-channel kernel takes from the records (merged about one pivot, as it does)
    mean, var = s1 / m, g.var(dim=0, unbiased=False)
    r = part.double()
    P = r[0, :, 2]
    d = r[..., 2] - P
    S1 = (r[..., 0] + r[..., 3] * d).sum(0)
    S2 = (r[..., 1] + 2 * d * r[..., 0] + r[..., 3] * d * d).sum(0)
    mean_k, var_k = S1 / m + P, S2 / m - (S1 / m) ** 2
    em = ((mean_k - mean).abs() / var.sqrt()).max().item()
    ev = ((var_k - var).abs() / var).max().item()
    print(f"conv1x1 narrow moments m={m} k={k} n={n} rows={rows}: sum {e1:.2e} sumsq {e2:.2e} mean/sigma {em:.2e} var {ev:.2e}")
    assert e1 < 1e-5
    assert e2 < 1e-5
    assert em < 1e-5
    assert ev < 1e-5


@pytest.mark.parametrize("batch", [256, "ragged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_narrow_gemm_moment_records(shape, batch):
    from mrla_amd import _lib as L
    h, w_, k, n = shape
    if batch == "ragged":
        m = _ragged_m(256 * h * w_, k, n)
        assert m % 32
    else:
        m = batch * h * w_
    upw, depth, _, _ = L.conv1x1_plan(m, k, n)
    assert depth == 2 and upw > depth, (upw, depth)    # the narrow form, its register double buffer refilled
    _check(m, k, n, seed=5000 + k + n)


@pytest.mark.parametrize("k", [64, 128, 256])
def test_pixel_waves_without_a_block(k):
    """70 pixels = 3 blocks (the last one ragged) for ONE workgroup of 4 (k <= 128) or 8 (k = 256) pixel-waves at n = 64:
    the waves past the third never enter the block loop and publish records with count 0."""
    from mrla_amd import _lib as L
    m, n = 70, 64
    upw, _, wgs, rows = L.conv1x1_plan(m, k, n)
    assert (upw, wgs, rows) == (1, 1, 1) and (m + 31) // 32 < 4
    _check(m, k, n, seed=6000 + k)
