"""The kernel instances of the 1x1-convolution GEMMs that no other test launches, each launched once, on integers, and
compared bit for bit.

The launchers (conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip, conv1x1_f32.hip) turn a plan into
template arguments: narrow <KS, MOM, NW>, wide <KS, MOM, ADD, SP>, K-streaming <WN, PB, MOM, ADD> and its 256 x 256 form,
the weight-gradient tiles <TN, TK>, the fp32 forms -- each as a bf16 and an fp16 kernel.  A transposed argument in that
dispatch is wrong only at the shapes that select the instance.  profiles/conv1x1_shared.md lists the 148 instances the
dispatches can reach and the 138 of them the rest of the suite launches; the cases here are the other ten, each at the
smallest shape that selects it, which the case asserts from the library's plan queries.

No tolerance: x and the addend are in {-1, 0, 1} and a weight row has eight entries of +-1 spread over the reduction.  Every
product, partial sum, rounded output and moment record is then an integer the number formats hold exactly, whatever the
order of summation; the test computes the worst-case magnitudes in int64 and asserts that, and the expected values are an
int64 product on the CPU.  Moment records are compared through what the BatchNorm makes of them, the per-channel pixel
count, sum and sum of squares, merged in int64 (how a form cuts the pixels into record rows is its own affair)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NNZ = 8                                            # entries of +-1 per weight row
EXACT = {"bf16": 1 << 8, "f16": 1 << 11, "f32": 1 << 24}      # integers up to here are exact in the format


def _P(t):
    """(the caller keeps `t` alive until it has synchronised: a freed tensor's memory goes to the next allocation)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _trits(gen, *shape):
    return torch.randint(-1, 2, shape, generator=gen, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _product(m, k, n):
    """x [m, k] in {-1, 0, 1}, w [n, k] with NNZ entries of +-1 per row (one in every k / NNZ wide stretch of the row) and
    x w^T, all int64 on the CPU; computed once per shape and shared by the cases that use it."""
    gen = torch.Generator().manual_seed(m * 31 + k * 7 + n)
    x = _trits(gen, m, k)
    at = torch.arange(NNZ) * (k // NNZ) + torch.randint(0, k // NNZ, (n, NNZ), generator=gen)
    sign = torch.randint(0, 2, (n, NNZ), generator=gen) * 2 - 1
    w = torch.zeros(n, k, dtype=torch.int64).scatter_(1, at, sign)
    y = torch.zeros(m, n, dtype=torch.int64)
    for j in range(NNZ):                           # (the product through w's entries: an int64 matmul has no fast path)
        y += x[:, at[:, j]] * sign[:, j]
    assert int(w.abs().sum(1).max()) == NNZ        # so that |any partial sum| <= NNZ
    return x, w, y


def _cuda(t, td):
    return t.to(td).cuda().contiguous()


def _filled(shape, td):
    return torch.full(shape, float("nan"), dtype=td, device="cuda")


def _assert_moments(part, y):
    """part [rows, n, 4] = (sum (y - p), sum (y - p)^2, p, count) per record row; y int64 [m, n] the rounded outputs"""
    m = y.shape[0]
    assert int(m * (2 * y.abs().max()) ** 2) < EXACT["f32"]    # every sum a record can hold is an exact fp32 integer
    p = part.double().cpu()
    assert torch.isfinite(p).all() and torch.equal(p, p.round())
    s1, s2, pv, cnt = (p[..., i].to(torch.int64) for i in range(4))
    assert torch.equal(cnt.sum(0), torch.full_like(cnt[0], m))
    assert torch.equal((s1 + cnt * pv).sum(0), y.sum(0))
    assert torch.equal((s2 + 2 * pv * s1 + cnt * pv * pv).sum(0), (y * y).sum(0))


# ---- the 16-bit forward forms: (m, k, n) of an instance.  The larger K-streaming pixel tile (PB = 2) needs 300 workgroups,
# the 256 x 256 tile 70 % of a round of 256 ----
FWD = {"narrow-ks16": (300, 256, 64), "wide-ks8": (300, 128, 256), "kstream-wn2-pb2": (4865, 512, 1920),
       "kstream-wn4-pb2": (4737, 512, 2048), "kstream-256": (5633, 1024, 2048)}
# epilogues: records = mrla_conv1x1_fwd with moment records; addend = mrla_conv1x1_fwd_addend, compact-addend = with the
# gradient of a stride-2 subsample; add = mrla_conv1x1_fwd_add, the wide form's addition in fp32 before the one rounding
FWD_CASES = [("kstream-wn2-pb2", "bf16", "addend"), ("kstream-wn2-pb2", "f16", "addend"), ("kstream-wn2-pb2", "f16", "records"),
             ("kstream-wn4-pb2", "f16", "addend"), ("kstream-256", "f16", "addend"), ("narrow-ks16", "f16", "addend"),
             ("wide-ks8", "f16", "add"), ("wide-ks8", "f16", "compact-addend")]


def _instance(m, k, n, dt):
    """The name of the instance the library's plan queries say (m, k, n) takes."""
    from mrla_amd import _lib as L
    plan = L.conv1x1_plan(m, k, n, dtype=dt)
    if L.load().mrla_conv1x1_add_supported(m, k, n, dt) == 1:
        return f"wide-ks{k // 16}"
    if k <= 256:
        return f"narrow-ks{k // 16}"
    if plan[1] == 4:
        return "kstream-256"
    wn = 4 if n % 256 == 0 else 2
    pb = [p for p in (1, 2) if plan[3] == -(-m // (8 // wn * p * 32))]
    assert len(pb) == 1                            # the record rows tell the two pixel tiles apart at this m
    return f"kstream-wn{wn}-pb{pb[0]}"


@pytest.mark.parametrize("name, dtype, epilogue", FWD_CASES, ids=["-".join(c) for c in FWD_CASES])
def test_forward_instance(name, dtype, epilogue):
    from mrla_amd import _lib as L
    m, k, n = FWD[name]
    td, dt = {"bf16": (torch.bfloat16, L.BF16), "f16": (torch.float16, L.F16)}[dtype]
    assert _instance(m, k, n, dt) == name
    x, w, y = _product(m, k, n)
    xt, wt, out, part = _cuda(x, td), _cuda(w, td), _filled((m + 8, n), td), None
    if epilogue == "records":
        part = _filled((L.load().mrla_conv1x1_rows(m, k, n, dt), n, 4), torch.float32)
        L.call("mrla_conv1x1_fwd", _P(xt), _P(wt), _P(out), _P(part), m, k, n, dt, _stream())
    else:
        # m = 1 * h * wd; compact: the gradient of x[:, :, ::2, ::2], whose pixel (yc, xc) belongs to output pixel (2 yc, 2 xc)
        h = next(d for d in (3, 7, 43) if m % d == 0)
        wd, s = m // h, 2 if epilogue == "compact-addend" else 1
        a = _trits(torch.Generator().manual_seed(len(name)), -(-h // s), -(-wd // s), n)
        full = torch.zeros(h, wd, n, dtype=torch.int64)
        full[::s, ::s] = a
        y = y + full.view(m, n)
        at = _cuda(a, td)
        if epilogue == "add":
            L.call("mrla_conv1x1_fwd_add", _P(xt), _P(wt), _P(at), _P(out), m, k, n, dt, _stream())
        else:
            L.call("mrla_conv1x1_fwd_addend", _P(xt), _P(wt), _P(at), _P(out), m, k, n, 1, h, wd, s, s, dt, _stream())
    torch.cuda.synchronize()
    assert int(y.abs().max()) <= NNZ + 1 <= EXACT[dtype]
    assert torch.isnan(out[m:].float()).all(), "a row at or past m was stored"
    assert torch.equal(out[:m].cpu().double(), y.double())
    if part is not None:
        _assert_moments(part, y)


@pytest.mark.parametrize("records", [False, True], ids=["plain", "records"])
def test_fp32_forward_with_streamed_weights_and_one_channel_group(records):
    """conv1x1_f32_fwd_kernel<1, MOM, true>: plan form 4 (k > 256, n = 64)"""
    from mrla_amd import _lib as L
    m, k, n = 300, 512, 64
    assert L.conv1x1_f32_plan(m, k, n)[0] == 4
    x, w, y = _product(m, k, n)
    xt, wt, out = _cuda(x, torch.float32), _cuda(w, torch.float32), _filled((m + 8, n), torch.float32)
    part = _filled((L.load().mrla_conv1x1_f32_rows(m, k, n), n, 4), torch.float32) if records else None
    L.call("mrla_conv1x1_f32_fwd", _P(xt), _P(wt), 0, _P(out), _P(part), m, k, n, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(out[m:]).all() and torch.equal(out[:m].cpu().double(), y.double())
    if records:
        _assert_moments(part, y)
