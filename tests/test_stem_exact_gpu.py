"""Exact check of the fused stem tail's three kernels (mrla_bn_relu_pool_fwd / _dmoments / _bwd, driven through the C ABI)
against a float64 CPU restatement, with guard regions around every tensor the kernels touch.

Inputs lie on dyadic grids chosen so that EVERY fp32 operation of the kernels is exact: sc*x + sh, the window maxima, the band
sums (integers of a fixed grid unit, far below 2^24 units) and cb0*dz + cb1*x + cb2.  The only rounding left is the single
conversion to the tensor type, so the float64 reference, rounded once to that type, must match BIT FOR BIT: there is no
tolerance in this file.  Two families: `coarse` (halves: many ties between window positions, many windows whose maximum is 0)
and `fine` (x in eighths, sc in 64ths: the bf16 / fp16 rounding of the activation really rounds, so a kernel that took the
maximum on unrounded values would route gradients differently).

Every device tensor is a view into a larger flat tensor with at least one whole image in front of and behind it.  Outputs
(out, dx, tmom) and their guards are prefilled with a NaN bit pattern: afterwards the guards must be untouched (compared as
integers) and no payload element may still hold the pattern.  The guards of the inputs (x, dP) hold 2^14: a read outside the
tensor would win a window or show up in a sum.

Shapes: every path of the row-band / strip geometry -- bands that divide Ho unevenly (65 .. 258 rows: with the former
ceil(Ho / bands) split their trailing bands were empty and the backward kernel stored rows of the next image), 32 bands, one
output column, more strips than waves with a ragged last strip, odd sizes, two and three channel groups, the 2x2 minimum."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 66, 4), (1, 64, 65, 8), (1, 64, 70, 4), (1, 64, 82, 4), (1, 64, 258, 32),      # unevenly divided bands
          (2, 64, 66, 8),            # ... where a row past an image is a row of the next image
          (1, 64, 256, 2),           # 32 bands, Wo = 1
          (1, 64, 4, 70),            # 9 strips for 8 waves, ragged last strip
          (2, 64, 16, 16), (3, 64, 15, 17), (2, 64, 7, 5), (1, 64, 2, 2), (2, 128, 9, 22), (1, 192, 30, 34)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
NAN_BITS = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float16: 0x7E5A}     # quiet NaNs with a payload
GUARD_VALUE = float(2 ** 14)


def _randint(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def _inputs(shape, family):
    """float64 CPU tensors on the grids of the module docstring: x, dP as [b, c, *, *]; per-channel sc, sh, cb[c, 3], center."""
    b, c, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + c + b + (0 if family == "coarse" else 500000))
    if family == "coarse":
        x = _randint(gen, -8, 8, shape) / 2
        sc = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[torch.randint(0, 6, (c,), generator=gen)]
        sh = _randint(gen, -4, 4, (c,)) / 2
    else:
        x = _randint(gen, -32, 32, shape) / 8
        # sc = j/64 in [-1, 2], never 0, sh = j/4 in [-2, 2]: a fixed set of pairs spread evenly over both grids, shuffled over
        # the channels, rather than independent draws -- how many activations the tensor type rounds depends on the (sc, sh)
        # pairs (fp16 rounds only values >= 4), and with 64 independent draws that fraction swings between 0.9 % and 2.8 %
        # from shape to shape; over these pairs and the grid of x it is 1.6 - 1.8 % (fp16) and 22 - 23 % (bf16)
        i = torch.randperm(c, generator=gen)
        j = (i.double() * (192 / c)).floor() - 64
        sc = torch.where(j >= 0, j + 1, j) / 64
        sh = ((i * 11) % 17 - 8).double() / 4
    dp = _randint(gen, -32, 32, (b, c, ho, wo)) / 8
    cb = torch.stack([torch.tensor([0.5, 1.0, -0.75], dtype=torch.float64)[torch.randint(0, 3, (c,), generator=gen)],
                      _randint(gen, -16, 16, (c,)) / 16, _randint(gen, -16, 16, (c,)) / 8], dim=1)
    center = _randint(gen, -8, 8, (c,)) / 4
    return x, dp, sc, sh, cb, center


def _round(v, dtype):
    """float64 -> the tensor type -> float64.  The values are fp32 numbers already (asserted by the caller), so the step through
    fp32 rounds nothing and the conversion to `dtype` is the one rounding (to nearest even, as the kernels' from_f)."""
    v32 = v.float()
    assert torch.equal(v32.double(), v)
    return v32.to(dtype).double()


@functools.lru_cache(maxsize=None)
def _reference(shape, family, dname):
    """Everything the kernels compute, in float64 on the CPU; computed once per case and shared, never modified."""
    dtype = DTYPES[dname]
    b, c, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x, dp, sc, sh, cb, center = _inputs(shape, family)
    per = lambda v: v.view(1, c, 1, 1)  # noqa: E731
    pre = per(sc) * x + per(sh)
    # the fp32 restatement (product, then sum: two roundings where the kernel's fma has one) gives the same numbers: exact
    assert torch.equal((per(sc).float() * x.float() + per(sh).float()).double(), pre)
    act = torch.relu(pre)
    a = _round(act, dtype)
    # windows: pad with -1 (a >= 0 and a window's centre always exists, so a padded position is never the maximum); the first
    # position in row-major scan order that holds the maximum
    win = F.pad(a, (1, 1, 1, 1), value=-1.0).unfold(2, 3, 2).unfold(3, 3, 2).reshape(b, c, ho, wo, 9)
    assert win.shape[2:4] == (ho, wo)
    m = win.max(dim=-1).values
    k = torch.where(win == m.unsqueeze(-1), torch.arange(9), torch.tensor(9)).min(dim=-1).values
    assert int(k.max()) < 9 and torch.equal(k, win.argmax(dim=-1))
    rows = 2 * torch.arange(ho).view(1, 1, ho, 1) - 1 + k // 3
    cols = 2 * torch.arange(wo).view(1, 1, 1, wo) - 1 + k % 3
    assert int(rows.min()) >= 0 and int(rows.max()) < h and int(cols.min()) >= 0 and int(cols.max()) < w
    flat = rows * w + cols
    m_aten, flat_aten = F.max_pool2d(a, 3, 2, 1, return_indices=True)        # ATen's CPU kernel: same maxima, same positions
    assert torch.equal(m_aten, m) and torch.equal(flat_aten, flat)
    g = torch.where(m > 0, dp, torch.zeros_like(dp))                          # a window whose maximum is 0 passes nothing
    dz = torch.zeros(b, c, h * w, dtype=torch.float64).scatter_add_(2, flat.view(b, c, -1), g.view(b, c, -1)).view(b, c, h, w)
    dx = _round(per(cb[:, 0]) * dz + per(cb[:, 1]) * x + per(cb[:, 2]), dtype)
    xk = x.view(b, c, h * w).gather(2, flat.view(b, c, -1)).view(b, c, ho, wo)
    # per window row: sum dz, sum dz*x, sum dz*(x - center)   [b, c, ho]
    s0, s1, s1c = g.sum(-1), (g * xk).sum(-1), (g * (xk - per(center))).sum(-1)
    # exactness of the kernels' fp32 sums: every term is an integer number of 1/64 (dP in 1/8 times x in 1/8; center in 1/4),
    # every partial sum of a band is bounded by the sum of the magnitudes below, and fp32 holds integers up to 2^24
    assert ho * wo < 16384
    units = 64 * (g.abs() * (xk.abs() + per(center).abs())).sum(dim=(2, 3)).max().item()
    assert units < 2 ** 24 and units == int(units)
    nwin = b * c * ho * wo
    stats = dict(ties=((win == m.unsqueeze(-1)).sum(-1)[m > 0] > 1).sum().item() / nwin, zero=(m == 0).sum().item() / nwin,
                 rounded=(a != act).double().mean().item())
    return dict(out=m, dx=dx, s0=s0, s1=s1, s1c=s1c, stats=stats)


def _check_input_strength(family, dname, stats):
    """The inputs exercise what they are for (conditions on the reference alone, not measurements of the kernels)."""
    if family == "coarse":
        assert stats["ties"] >= 0.05, stats           # windows with a positive maximum at more than one position
        assert stats["zero"] >= 0.02, stats           # windows whose maximum is 0
    elif dname != "f32":
        assert stats["rounded"] >= (0.10 if dname == "bf16" else 0.01), stats     # activations the tensor type really rounds


class _Guarded:
    """A payload of `n` elements inside a larger flat device tensor: `guard` (>= 1, rounded up to a multiple of 64 elements so
    that the payload starts 16-byte aligned) elements in front and behind."""

    def __init__(self, n, guard, dtype, values=None):
        self.n, self.g, self.dtype = n, -(-guard // 64) * 64, dtype
        self.flat = torch.empty(self.n + 2 * self.g, dtype=dtype, device="cuda")
        self.payload = self.flat[self.g:self.g + n]
        assert self.payload.data_ptr() % 16 == 0 and self.g >= guard >= 1
        if values is None:                      # an output: NaN pattern everywhere
            self.flat.view(INT_OF[dtype]).fill_(self._pattern())
        else:                                   # an input: 2^14 around the values
            self.flat.fill_(GUARD_VALUE)
            self.payload.copy_(values.reshape(-1).to(dtype))
            assert torch.equal(self.payload.double().cpu(), values.reshape(-1))        # the grid values are exact in `dtype`

    def _pattern(self):
        bits = NAN_BITS[self.dtype]
        return bits - (1 << 32) if bits >= 1 << 31 else bits

    def ptr(self):
        return self.payload.data_ptr()

    def check_output(self, what):
        ints = self.flat.view(INT_OF[self.dtype])
        pat = self._pattern()
        front, back, body = ints[:self.g], ints[self.g + self.n:], ints[self.g:self.g + self.n]
        assert bool((front == pat).all()), f"{what}: write in front of the tensor"
        assert bool((back == pat).all()), f"{what}: write behind the tensor"
        assert not bool((body == pat).any()), f"{what}: {int((body == pat).sum())} elements never written"
        return self.payload.cpu()


def _bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("family", ["coarse", "fine"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_kernels_match_the_float64_reference_bit_for_bit_inside_guards(shape, family, dname):
    from mrla_amd import _lib as L, functional as Fm
    dtype, dt = DTYPES[dname], Fm._DT[DTYPES[dname]]
    b, c, h, w = shape
    ref = _reference(shape, family, dname)
    print(f"{shape} {family} {dname}: {ref['stats']}")
    _check_input_strength(family, dname, ref["stats"])
    ho, wo, bands, waves, _, _ = L.bn_pool_plan(b, c, h, w, dt, 0)
    rows = L.load().mrla_bn_pool_rows(b, c, h, w, dt, L.NHWC)
    assert (ho, wo) == tuple(ref["out"].shape[2:]) and rows == b * bands
    if shape == (1, 64, 4, 70):
        assert waves == 8 and -(-wo // 4) == 9 and wo % 4 != 0
    if shape == (1, 64, 256, 2):
        assert bands == 32 and wo == 1
    band_rows = [L.bn_pool_plan(b, c, h, w, dt, i)[4:] for i in range(bands)]
    assert band_rows[0][0] == 0 and band_rows[-1][1] == ho and all(lo < hi for lo, hi in band_rows)

    x, dp, sc, sh, cb, center = _inputs(shape, family)
    image, oimage = h * w * c, ho * wo * c
    gx = _Guarded(b * image, image, dtype, _nhwc(x))
    gdp = _Guarded(b * oimage, oimage, dtype, _nhwc(dp))
    gout = _Guarded(b * oimage, max(oimage, image), dtype)
    gdx = _Guarded(b * image, image, dtype)
    gt0 = _Guarded(rows * c * 2, rows * c * 2, torch.float32)            # center = NULL
    gt1 = _Guarded(rows * c * 2, rows * c * 2, torch.float32)
    dev32 = lambda v: v.float().contiguous().cuda()  # noqa: E731
    sc_d, sh_d, cb_d, cen_d = dev32(sc), dev32(sh), dev32(cb), dev32(center)
    assert torch.equal(cb_d.double().cpu(), cb) and torch.equal(sc_d.double().cpu(), sc)
    st, geo = Fm._stream(), (b, c, h, w, dt, L.NHWC)
    L.call("mrla_bn_relu_pool_fwd", gx.ptr(), sc_d.data_ptr(), sh_d.data_ptr(), gout.ptr(), *geo, st)
    L.call("mrla_bn_relu_pool_dmoments", gdp.ptr(), gx.ptr(), sc_d.data_ptr(), sh_d.data_ptr(), None, gt0.ptr(), *geo, st)
    L.call("mrla_bn_relu_pool_dmoments", gdp.ptr(), gx.ptr(), sc_d.data_ptr(), sh_d.data_ptr(), cen_d.data_ptr(), gt1.ptr(), *geo, st)
    L.call("mrla_bn_relu_pool_bwd", gdp.ptr(), gx.ptr(), sc_d.data_ptr(), sh_d.data_ptr(), cb_d.data_ptr(), gdx.ptr(), *geo, st)
    torch.cuda.synchronize()

    out = gout.check_output("out").view(b, ho, wo, c).permute(0, 3, 1, 2)
    dx = gdx.check_output("dx").view(b, h, w, c).permute(0, 3, 1, 2)
    t0 = gt0.check_output("tmom").double().view(b, bands, c, 2)
    t1 = gt1.check_output("tmom (centered)").double().view(b, bands, c, 2)
    for name, got, want in (("out", out, ref["out"]), ("dx", dx, ref["dx"])):
        bad = _bits(got) != _bits(want.to(dtype))
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
    for name, t, second in (("tmom", t0, ref["s1"]), ("tmom (centered)", t1, ref["s1c"])):
        assert torch.equal(t.sum(1)[..., 0], ref["s0"].sum(-1)) and torch.equal(t.sum(1)[..., 1], second.sum(-1)), name
        for i, (lo, hi) in enumerate(band_rows):
            assert torch.equal(t[:, i, :, 0], ref["s0"][:, :, lo:hi].sum(-1)), (name, "sum dz", i)
            assert torch.equal(t[:, i, :, 1], second[:, :, lo:hi].sum(-1)), (name, "sum dz*x", i)
