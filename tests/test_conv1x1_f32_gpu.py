"""The fp32 1x1-convolution GEMMs on the fp32-input MFMA (mrla_conv1x1_f32_fwd / mrla_conv1x1_f32_wgrad) through the C ABI.

Every output (y, the moment records, the weight gradient's partial tiles and dw) sits inside a NaN-patterned guard region
that must be intact afterwards, with no payload element left unwritten.
  * exact: operands from {-4 .. 4} / 4.  Every product is a multiple of 2^-4 of magnitude <= 1 and every partial sum is at
    most 2048 (forward, k <= 2048) or 3141 (weight gradient, m <= 3141) in magnitude: 16 bits, so fp32 arithmetic is exact
    in any order (checked on the CPU below) and the kernels must equal the float64 product bit for bit;
  * random normal operands: |y - y64| <= (k + 1) 2^-24 sum_j |x_j| |w_j| per element ((m + 1) 2^-24 sum_p |dy_p| |x_p| for
    dw) -- the bound of a chain of k fused multiply-adds (plus a reduction) in any order, derived, not tuned;
  * records: raw sums recovered from them against float64 sums of the y the kernel stored (relmax < 1e-5, the bound
    tests/test_conv1x1_gpu.py puts on the same quantities), one case with the channel means 1000 sigma away at the bounds of
    test_conv_bn_statistics_when_the_mean_dwarfs_sigma (mean 1e-5, variance 1e-4), and mom_part = NULL: the same y;
  * two runs of each entry point are bit-equal, `part` included."""
import functools
import zlib

import numpy as np
import pytest
import torch

from tests.test_light_gpu import relmax
from tests.test_stem_exact_gpu import _Guarded, _bits

pytestmark = pytest.mark.gpu

# (m, k, n, w_trans): the m x (k, n) cross of the specification, thinned -- every (k, n) at least once, every m with the smallest and the
# largest k, both weight layouts in every kernel form; (512, 64) is added for the streaming form with one channel group
CASES = [(1, 64, 64, 0), (1, 2048, 512, 1), (1, 64, 256, 1),
         (33, 64, 256, 0), (33, 2048, 512, 0), (33, 256, 64, 1), (33, 128, 512, 0),
         (98, 64, 64, 1), (98, 2048, 512, 1), (98, 512, 128, 0), (98, 256, 1024, 1), (98, 1024, 2048, 0), (98, 512, 64, 0),
         (3141, 64, 256, 0), (3141, 2048, 512, 0), (3141, 128, 512, 1), (3141, 512, 2048, 1), (3141, 1024, 256, 0),
         (3141, 256, 1024, 0), (3141, 512, 64, 1), (3141, 64, 64, 0), (3141, 256, 64, 0)]
WGRAD_CASES = sorted({(m, k, n) for m, k, n, _ in CASES})
FORMS = {0, 1, 2, 4, 5}          # mrla_conv1x1_f32_plan: resident weights x {1, 2, 4} channel groups, streamed x {1, 2}


def _id(c):
    return "x".join(map(str, c))


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def _operands(family, shape, gen):
    if family == "exact":
        return torch.randint(-4, 5, shape, device="cuda", generator=gen).float() / 4
    return torch.randn(shape, device="cuda", generator=gen)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _fp32_sums_of_grid_products_are_exact():
    """float32 running sums of products of {-4..4}/4 values equal the float64 ones, in several orders, up to 3141 terms."""
    rng = np.random.default_rng(7)
    a, b = rng.integers(-4, 5, 3141) / 4.0, rng.integers(-4, 5, 3141) / 4.0
    for prod in (a * b, np.ones(3141), -np.ones(3141), np.abs(a * b)):
        for order in (np.arange(3141), np.arange(3141)[::-1], rng.permutation(3141), np.argsort(prod), np.argsort(-prod)):
            p = prod[order]
            c32 = np.cumsum(p.astype(np.float32), dtype=np.float32)
            assert np.array_equal(c32.astype(np.float64), np.cumsum(p))
            # ... and as a chain of fused multiply-adds: the product itself is exact in fp32 too
            assert np.array_equal((a.astype(np.float32) * b.astype(np.float32)).astype(np.float64), a * b)
    return True


def _run_fwd(x, w, w_trans, m, k, n, moments=True):
    from mrla_amd import _lib as L
    lib = L.load()
    rows = lib.mrla_conv1x1_f32_rows(m, k, n)
    assert rows > 0
    y = _Guarded(m * n, 4096, torch.float32)
    part = _Guarded(rows * n * L.GEMM_MOMENTS, 4096, torch.float32) if moments else None
    rc = lib.mrla_conv1x1_f32_fwd(x.data_ptr(), w.data_ptr(), w_trans, y.ptr(), part.ptr() if moments else None, m, k, n,
                                  _stream())
    assert rc == L.OK
    torch.cuda.synchronize()
    yv = y.check_output("y").view(m, n)
    pv = part.check_output("mom_part").view(rows, n, L.GEMM_MOMENTS) if moments else None
    return yv, pv


def _run_wgrad(dy, x, m, k, n):
    from mrla_amd import _lib as L
    lib = L.load()
    rows = lib.mrla_conv1x1_f32_wgrad_rows(m, k, n)
    assert rows > 0
    part = _Guarded(rows * n * k, 4096, torch.float32)
    dw = _Guarded(n * k, 4096, torch.float32)
    rc = lib.mrla_conv1x1_f32_wgrad(dy.data_ptr(), x.data_ptr(), part.ptr(), dw.ptr(), m, k, n, _stream())
    assert rc == L.OK
    torch.cuda.synchronize()
    return dw.check_output("dw").view(n, k), part.check_output("part")


def _raw_sums(part):
    r = part.double()
    s1, s2, p, cnt = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    return (s1 + cnt * p).sum(0), (s2 + 2 * p * s1 + cnt * p * p).sum(0)


def test_the_cases_reach_every_kernel_form():
    from mrla_amd import _lib as L
    seen = {}
    for m, k, n, t in CASES:
        plan = L.conv1x1_f32_plan(m, k, n)
        assert plan is not None and plan[3] == L.load().mrla_conv1x1_f32_rows(m, k, n)
        seen.setdefault(plan[0], set()).add(t)
    assert set(seen) == FORMS, seen
    assert all(v == {0, 1} for v in seen.values()), seen          # both weight layouts in every form
    # several pixel groups per persistent workgroup, in a resident and in a streaming form
    multi = set()
    for m, k, n, _ in CASES:
        form, _, _, rows = L.conv1x1_f32_plan(m, k, n)
        pixel_waves = 4 // (1, 2, 4)[form & 3]
        groups = -(-(-(-m // 32)) // pixel_waves)
        if groups > rows:
            multi.add(form >= 4)
    assert multi == {False, True}, multi


@pytest.mark.parametrize("family", ["exact", "normal"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_input_gradient_product(case, family):
    m, k, n, w_trans = case
    g = _gen("fwd", case, family)
    x = _operands(family, (m, k), g)
    w = _operands(family, (n, k), g)                       # [n, k]; handed over as [k, n] with w_trans
    w_arg = w.t().contiguous() if w_trans else w
    y, part = _run_fwd(x, w_arg, w_trans, m, k, n)
    y64 = x.double() @ w.double().t()
    if family == "exact":
        assert _fp32_sums_of_grid_products_are_exact()
        assert torch.equal(y.double(), y64.cpu()), (y.double() - y64.cpu()).abs().max().item()
    else:
        bound = (k + 1) * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t())
        excess = ((y.double() - y64.cpu()).abs() - bound.cpu()).max().item()
        print(f"fwd {case}: max |err| / bound = {((y.double() - y64.cpu()).abs() / bound.cpu()).max().item():.3g}")
        assert excess <= 0, excess
    # the records are those of the y that was stored
    s1, s2 = _raw_sums(part)
    assert part[:, :, 3].double().sum(0).eq(m).all()
    yd = y.double()
    print(f"records {case}: {relmax(s1.numpy(), yd.sum(0).numpy()):.3g} {relmax(s2.numpy(), (yd * yd).sum(0).numpy()):.3g}")
    assert relmax(s1.numpy(), yd.sum(0).numpy()) < 1e-5 and relmax(s2.numpy(), (yd * yd).sum(0).numpy()) < 1e-5
    # no records wanted: the same y; and a second run of both: the same bits
    y2, _ = _run_fwd(x, w_arg, w_trans, m, k, n, moments=False)
    y3, part3 = _run_fwd(x, w_arg, w_trans, m, k, n)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(y), _bits(y3)) and torch.equal(_bits(part), _bits(part3))


@pytest.mark.parametrize("family", ["exact", "normal"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_id)
def test_weight_gradient(case, family):
    m, k, n = case
    g = _gen("wgrad", case, family)
    dy = _operands(family, (m, n), g)
    x = _operands(family, (m, k), g)
    dw, part = _run_wgrad(dy, x, m, k, n)
    dw64 = (dy.double().t() @ x.double()).cpu()
    if family == "exact":
        assert _fp32_sums_of_grid_products_are_exact()
        assert torch.equal(dw.double(), dw64), (dw.double() - dw64).abs().max().item()
    else:
        bound = ((m + 1) * 2.0 ** -24 * (dy.double().abs().t() @ x.double().abs())).cpu()
        print(f"wgrad {case}: max |err| / bound = {((dw.double() - dw64).abs() / bound).max().item():.3g}")
        assert ((dw.double() - dw64).abs() - bound).max().item() <= 0
    dw2, part2 = _run_wgrad(dy, x, m, k, n)
    assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(part), _bits(part2))


def test_records_when_the_mean_dwarfs_sigma():
    """y[m, c] = mean_c (1 + noise / 1000), |mean_c| in 64 .. 120: the records, merged in double about one pivot as
    mrla_bn_stats_fwd_rows merges them, give the batch mean to 1e-5 and the variance to 1e-4 of the float64 statistics of
    the stored y (raw one-pass fp32 sums would lose eps * ratio^2 = 6 % of the variance)."""
    m, k, n, ratio = 3141, 64, 256, 1000.0
    g = _gen("dwarf")
    x = 1.0 + torch.randn((m, k), device="cuda", generator=g) * (k ** 0.5) / ratio
    sign = 2 * (torch.rand((n,), device="cuda", generator=g) > 0.5).float() - 1
    means = (64 + 56 * torch.rand((n,), device="cuda", generator=g)) * sign
    w = (means[:, None] / k).expand(n, k).contiguous()
    y, part = _run_fwd(x, w, 0, m, k, n)
    yd = y.double()
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    assert (mean.abs() / var.sqrt()).median().item() >= 0.9 * ratio
    r = part.double()
    s1, s2, p, cnt = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    d = p - p[0]                                            # re-base every row onto the first row's pivot
    S1 = (s1 + cnt * d).sum(0)
    S2 = (s2 + 2 * d * s1 + cnt * d * d).sum(0)
    gm = p[0] + S1 / m
    gv = S2 / m - (S1 / m) ** 2
    print(f"mean {((gm - mean).abs() / mean.abs()).max().item():.3g} var {((gv - var).abs() / var).max().item():.3g}")
    assert ((gm - mean).abs() / mean.abs()).max().item() < 1e-5
    assert ((gv - var).abs() / var).max().item() < 1e-4


def test_refusals_launch_nothing():
    from mrla_amd import _lib as L
    lib = L.load()
    buf = torch.zeros(64 * 64 + 16, device="cuda")
    p = buf.data_ptr()
    before = buf.clone()
    assert lib.mrla_conv1x1_f32_fwd(p, p, 0, p + 4, None, 1, 64, 64, _stream()) == L.EINVAL
    assert lib.mrla_conv1x1_f32_fwd(p, p, 0, None, None, 1, 64, 64, _stream()) == L.EINVAL
    assert lib.mrla_conv1x1_f32_fwd(p, p, 0, p, None, 1, 96, 64, _stream()) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_f32_wgrad(p, p, p, p + 4, 1, 64, 64, _stream()) == L.EINVAL
    assert lib.mrla_conv1x1_f32_wgrad(p, p, p, p, 1, 4096, 64, _stream()) == L.EUNSUPPORTED     # (m, k, n): k > 2048
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
