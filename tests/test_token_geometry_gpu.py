"""MRLA-light on tokens (tokens_nhwc.hip, tokens.hip) at the geometries and element types the other token tests do not reach,
against the float64 numpy oracle.

Geometry: the row kernels cut a map of `side` columns into strips of 7 (at most 8 waves: from side 57 on a wave takes a second
strip) and the forward cuts its rows into 1, 2 or 4 bands (token_bands); widths with c % 64 != 0 keep the whole map of a
16-channel chunk in LDS instead.  CASES holds the smallest shape that reaches each of these.

Element types: the light token path stores nothing 16-bit between its kernels (statistics, dxn and the partials are float32), so
each of out, dx and do is float32 arithmetic followed by ONE rounding.  With a = the kernel's float32 value and r = the oracle's,
round-to-nearest gives |rnd(a) - rnd(r)| <= |a - r| + ulp, and the float32 path is held to ACT_TOL of the tensor's maximum by the
float32 tests of this file, so per element
    |got - rnd(want64)| <= u * |rnd(want64)| + ACT_TOL * max|want64| + tiny
with u = 2^-7 (bf16) / 2^-10 (fp16) and tiny = 2^-24 (fp16's subnormal spacing): assert_storage_close, no outliers."""
import functools

import numpy as np
import pytest
import torch

from oracle import detgen
from tests import cases
from tests.test_light_gpu import ACT_TOL, par_tol, relmax, to_dev
from tests.test_stem_exact_gpu import _Guarded as Guarded
from tests.test_tokens_gpu import NAMES, ORACLE, oracle, run

pytestmark = pytest.mark.gpu

D = 16
CASES = {
    "side1": (3, 2, 64),            # 1 x 1 map: every tap but the centre is padding
    "side15": (2, 226, 64),         # 3 strips, the last one 1 column; 2 bands
    "side16": (1, 257, 64),         # last strip 2 columns; 4 bands of 4 rows
    "side17": (2, 290, 128),        # 4 uneven bands (4, 4, 4, 5); last strip 3 columns
    "side24": (1, 577, 192),        # DeiT-384 map: 4 strips, 4 bands of 6
    "side57": (1, 3250, 64),        # 9 strips on 8 waves: wave 0 takes a second strip
    "tile16": (2, 17, 16),          # LDS-tile path, one 16-channel chunk
    "tile48": (2, 82, 48),          # tile path, 3 chunks, c not a multiple of 32
    "tile80s30": (1, 901, 80),      # tile path at the largest side its backward serves
    "side4": (2, 17, 64),           # (16-bit cases only) one strip, one band
    "side14": (2, 197, 192),        # (fp16 only) the DeiT-224 map
    "side8": (3, 65, 768),          # (band independence) 2 bands as a batch of 3, 1 band inside a batch of 128
}
FP32_CASES = ("side1", "side15", "side16", "side17", "side24", "side57", "tile16", "tile48", "tile80s30")
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}
STORAGE_CASES = [(k, t) for t in STORAGE for k in ("side15", "side16", "side17", "side24", "tile48", "side4")] + [("side14", "fp16")]
DTYPES = {"fp32": torch.float32, **STORAGE}


def rnd(a, dtype):
    """float64 -> the storage type (to nearest even, as the kernels' from_f) -> float64."""
    if dtype == torch.float32:
        return np.asarray(a, np.float64)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).double().numpy()


def assert_storage_close(got, want64, dtype, what):
    """The bound of the module docstring; float32 tensors get the bound of the float32 tests (ACT_TOL of the maximum)."""
    want64 = np.asarray(want64, np.float64)
    if dtype == torch.float32:
        err = relmax(got, want64)
        print(f"{what}: {err:.3e} of max (bound {ACT_TOL:.1e})")
        assert err < ACT_TOL, what
        return
    u, tiny = (2.0 ** -7, 0.0) if dtype == torch.bfloat16 else (2.0 ** -10, 2.0 ** -24)
    want = rnd(want64, dtype)
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = u * np.abs(want) + ACT_TOL * np.abs(want64).max() + tiny
    bad = err > tol
    print(f"{what}: worst error / bound {(err / tol).max():.3f}")
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} beyond the rounding bound; worst {(err / tol).max():.2f} x the bound"


@functools.lru_cache(maxsize=None)
def problem(name, dname):
    """Inputs (rounded to the storage type) and parameters of a case: read-only, shared by the tests of that case."""
    b, n, c = CASES[name]
    s = detgen.seed_of(f"tok-geo/{name}")
    dtype = DTYPES[dname]
    x = rnd(detgen.normalish((b, n, c), s) * 1.4 + 0.25, dtype)
    o = rnd(detgen.normalish((b, n, c), s + 1) * 0.8 - 0.1, dtype)
    gup = rnd(detgen.normalish((b, n, c), s + 2), dtype)
    return x, o, gup, cases.token_params(c, salt=17)


@functools.lru_cache(maxsize=None)
def reference(name, dname, res):
    x, o, gup, P = problem(name, dname)
    return oracle(x, o, P, D, gup, res)


def check_params(pg, g):
    for got, key in zip(pg, ORACLE):
        err = relmax(np.asarray(got).ravel(), np.asarray(g[key]).ravel())
        print(f"{key}: {err:.3e} of max (bound {par_tol(key):.1e})")
        assert err < par_tol(key), key


# ------------------------------------------------------------------------------------------------
# (a) float32, every geometry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FP32_CASES)
@pytest.mark.parametrize("res", [False, True], ids=["module", "block"])
def test_token_geometry_fp32(name, res):
    x, o, gup, P = problem(name, "fp32")
    out, dx, do, pg = run(x, o, P, D, gup, torch.float32, res)
    want, g = reference(name, "fp32", res)
    assert relmax(out, want) < ACT_TOL
    assert relmax(dx, g["dxt"]) < ACT_TOL
    assert relmax(do, g["dot"]) < ACT_TOL
    for got, key in zip(pg, ORACLE):
        assert relmax(got.ravel(), np.asarray(g[key]).ravel()) < par_tol(key), key


# ------------------------------------------------------------------------------------------------
# (b) bf16 and fp16 storage
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dname", STORAGE_CASES, ids=[f"{k}-{t}" for k, t in STORAGE_CASES])
@pytest.mark.parametrize("res", [False, True], ids=["module", "block"])
def test_token_geometry_16bit(name, dname, res):
    dtype = STORAGE[dname]
    x, o, gup, P = problem(name, dname)
    out, dx, do, pg = run(x, o, P, D, gup, dtype, res)
    want, g = reference(name, dname, res)
    assert_storage_close(out, want, dtype, "out")
    assert_storage_close(dx, g["dxt"], dtype, "dx")
    assert_storage_close(do, g["dot"], dtype, "do")
    check_params(pg, g)


# ------------------------------------------------------------------------------------------------
# (c) the number of row bands changes nothing
# ------------------------------------------------------------------------------------------------
def run_tensors(x, o, P, gup, dtype, res=True):
    from mrla_amd.functional import mrla_token_light
    xt, ot = x.clone().requires_grad_(True), o.clone().requires_grad_(True)
    prm = [to_dev(P[k]).requires_grad_(True) for k in NAMES]
    out = mrla_token_light(xt, ot, *prm, D, eps=1e-6, res=res)
    out.backward(gup)
    torch.cuda.synchronize()
    return out.detach(), xt.grad, ot.grad, [p.grad.cpu().numpy() for p in prm]


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_token_forward_band_count_independent(dname):
    """(128, 65, 768): (C / 64) * B = 1536 workgroups, so token_bands gives ONE band; the same images as a batch of 3 get two.
    The per-pixel arithmetic does not depend on the band, and the backward is unbanded and per image: images 0, 77 and 127 of
    the large launch equal the batch of three bit for bit, and the batch of three matches the oracle."""
    dtype = DTYPES[dname]
    pick = [0, 77, 127]
    x3, o3, g3, P = problem("side8", dname)
    b, n, c = 128, *CASES["side8"][1:]
    gen = torch.Generator().manual_seed(20240611)
    big = [torch.randn((b, n, c), generator=gen).mul_(s).add_(m).to(dtype) for s, m in ((1.4, 0.25), (0.8, -0.1), (1.0, 0.0))]
    for t, small in zip(big, (x3, o3, g3)):
        t[pick] = torch.from_numpy(small).to(dtype)
    big = [t.cuda() for t in big]
    small = [t[pick].contiguous() for t in big]
    out_b, dx_b, do_b, _ = run_tensors(*big[:2], P, big[2], dtype)
    out_s, dx_s, do_s, pg = run_tensors(*small[:2], P, small[2], dtype)
    assert torch.equal(out_b[pick], out_s), "forward: 1 band and 2 bands differ"
    assert torch.equal(dx_b[pick], dx_s) and torch.equal(do_b[pick], do_s), "backward: a batch of 128 and of 3 differ"
    want, g = reference("side8", dname, True)
    assert_storage_close(out_s.float().cpu().numpy(), want, dtype, "out")
    assert_storage_close(dx_s.float().cpu().numpy(), g["dxt"], dtype, "dx")
    assert_storage_close(do_s.float().cpu().numpy(), g["dot"], dtype, "do")
    check_params(pg, g)


# ------------------------------------------------------------------------------------------------
# (d) every output element written, nothing outside touched
# ------------------------------------------------------------------------------------------------
def _guards(g):
    ints = g.flat.view({4: torch.int32, 2: torch.int16}[g.flat.element_size()])
    return ints[:g.g].clone(), ints[g.g + g.n:].clone()


@pytest.mark.parametrize("name", ["side16", "side57"])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_token_kernels_write_every_element_and_nothing_else(name, dname):
    """The six passes of the module through the C ABI, every tensor they touch inside guard regions (tests/test_stem_exact_gpu.py):
    outputs and their guards prefilled with a NaN bit pattern, input guards with 2^14.  A row band or a strip that nobody wrote
    shows up exactly, even where a comparison of values would read plausible stale memory."""
    from mrla_amd import _lib as L, functional as Fm
    dtype, dt = DTYPES[dname], Fm._DT[DTYPES[dname]]
    b, n, c = CASES[name]
    x, o, gup, P = problem(name, dname)
    want, g = reference(name, dname, True)
    image = n * c
    as64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    gx, go, gg = (Guarded(b * image, image, dtype, as64(a)) for a in (x, o, gup))
    gout, gdx, gdo = (Guarded(b * image, image, dtype) for _ in range(3))
    gdxn = Guarded(b * image, image, torch.float32)
    gstats = Guarded(b * n * 4, n * 4, torch.float32)
    prow = L.load().mrla_token_part_rows(b, n, c, dt)
    assert prow == b
    gpart = Guarded(prow * c * L.TOKEN_PARTIALS, c * L.TOKEN_PARTIALS, torch.float32)
    gbmom = Guarded(b * c * L.BWD_MOMENTS, c * L.BWD_MOMENTS, torch.float32)
    every = dict(x=gx, o_prev=go, dout=gg, out=gout, dx=gdx, do_prev=gdo, dxn=gdxn, stats=gstats, part=gpart, bmom=gbmom)
    before = {k: _guards(v) for k, v in every.items()}
    prm = {k: to_dev(P[k]).reshape(-1).contiguous() for k in NAMES}
    wxw, wxb, wow, wob = (prm[k].data_ptr() for k in ("normx.weight", "normx.bias", "normo.weight", "normo.bias"))
    wq, wk, wv, lam = (prm[k].data_ptr() for k in ("mrla.Wq.weight", "mrla.Wk.weight", "mrla.Wv.weight", "lambda_t"))
    ks = prm["mrla.Wq.weight"].numel()
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    mom, gate, dyx, dwqk = f32(b, c, L.FWD_MOMENTS), f32(b, c // D), f32(b, c), f32(b, 2 * ks)
    st, res = Fm._stream(), 1
    L.call("mrla_token_norm_pool", gx.ptr(), go.ptr(), wxw, wxb, 1e-6, gstats.ptr(), mom.data_ptr(), b, n, c, dt, st)
    L.call("mrla_light_gate_fwd", mom.data_ptr(), wq, wk, ks, gate.data_ptr(), b, c, n - 1, D, st)
    L.call("mrla_token_apply_fwd", gx.ptr(), go.ptr(), gstats.ptr(), wxw, wxb, wow, wob, wv, gate.data_ptr(), lam, gout.ptr(),
           b, n, c, D, res, dt, st)
    L.call("mrla_token_apply_bwd", gg.ptr(), gx.ptr(), go.ptr(), gstats.ptr(), wxw, wxb, wow, wob, wv, gate.data_ptr(), lam,
           gdxn.ptr(), gpart.ptr(), gbmom.ptr(), b, n, c, D, dt, st)
    L.call("mrla_token_gate_bwd", mom.data_ptr(), gbmom.ptr(), gate.data_ptr(), wq, wk, ks, dyx.data_ptr(), dwqk.data_ptr(),
           gpart.ptr(), b, n, c, D, dt, st)
    L.call("mrla_token_ln_bwd", gg.ptr(), gx.ptr(), go.ptr(), gdxn.ptr(), dyx.data_ptr(), gstats.ptr(), wxw, wow, lam, gdx.ptr(),
           gdo.ptr(), b, n, c, res, dt, st)
    torch.cuda.synchronize()
    for k, v in every.items():
        front, back = _guards(v)
        assert torch.equal(front, before[k][0]), f"{k}: write in front of the tensor"
        assert torch.equal(back, before[k][1]), f"{k}: write behind the tensor"
    got = {k: every[k].check_output(k) for k in ("out", "dxn", "dx", "do_prev", "stats", "part", "bmom")}
    assert_storage_close(got["out"].double().numpy().reshape(b, n, c), want, dtype, "out")
    assert_storage_close(got["dx"].double().numpy().reshape(b, n, c), g["dxt"], dtype, "dx")
    assert_storage_close(got["do_prev"].double().numpy().reshape(b, n, c), g["dot"], dtype, "do")


# ------------------------------------------------------------------------------------------------
# (e) refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n,c,d", [(2, 17, 24, 8), (1, 17, 1088, 16), (2, 18, 64, 16), (2, 17, 72, 16)],
                         ids=["c24-not-a-multiple-of-16", "c1088-beyond-64x16", "n18-no-square-map", "c72-not-a-multiple-of-d"])
def test_token_light_refuses_before_any_kernel(b, n, c, d, monkeypatch):
    from mrla_amd import _lib as L, functional as Fm
    entered = []
    monkeypatch.setattr(L, "call", lambda name, *a: entered.append(name))      # (functional launches through L.call only)
    x = torch.zeros((b, n, c), device="cuda")
    prm = [to_dev(v) for v in (cases.token_params(c, salt=17)[k] for k in NAMES)]
    with pytest.raises(L.MrlaHipError):
        Fm.mrla_token_light(x, x.clone(), *prm, d, eps=1e-6, res=True)
    assert entered == [], f"refused only after {entered}"


@pytest.mark.parametrize("sequences", [True, False], ids=["sequence-call", "per-pass-calls"])
def test_token_tile_side31_has_a_forward_and_no_backward(sequences, monkeypatch):
    """c % 64 != 0 keeps the map of a 16-channel chunk in LDS: one tile in the forward (side <= 46), two and the reduction
    scratch in the backward (side <= 30).  At c = 32, side 31 the forward is served and matches the oracle; the backward answers
    MRLA_EUNSUPPORTED, which surfaces as an MrlaHipError naming mrla_token_apply_bwd instead of as gradients."""
    from mrla_amd import _lib as L, functional as Fm
    monkeypatch.setattr(Fm, "SEQUENCES", sequences)
    b, n, c = 1, 962, 32
    s = detgen.seed_of("tok-geo/side31")
    x, o = detgen.normalish((b, n, c), s) * 1.4 + 0.25, detgen.normalish((b, n, c), s + 1) * 0.8 - 0.1
    P = cases.token_params(c, salt=17)
    xt, ot = to_dev(x).requires_grad_(True), to_dev(o).requires_grad_(True)
    prm = [to_dev(P[k]).requires_grad_(True) for k in NAMES]
    out = Fm.mrla_token_light(xt, ot, *prm, D, eps=1e-6, res=True)
    want, _ = oracle(x, o, P, D, np.zeros_like(x), True)
    assert relmax(out.detach().cpu().numpy(), want) < ACT_TOL
    with pytest.raises(L.MrlaHipError, match="mrla_token_apply_bwd") as info:
        out.backward(torch.ones_like(out))
    assert info.value.code == L.EUNSUPPORTED
    assert xt.grad is None and ot.grad is None and all(p.grad is None for p in prm)
