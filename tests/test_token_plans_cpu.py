"""Host-side answers of the token (DeiT) entry points: no kernel is launched, no GPU is needed.

mrla_token_part_rows sizes the `part` buffer of both token backward passes; mrla_token_base_supported decides whether a width
takes the fused MRLA-base token module (functional.token_base_supported).  The shapes are those of tests/test_token_geometry_gpu.py
and tests/test_token_base_geometry_gpu.py.  Also here, because it needs no GPU either: the rounding reference those 16-bit tests
compare against (oracle/token_base_storage.py) is pinned to the eager module it restates."""
import pytest

SIDES = (1, 2, 4, 5, 7, 8, 14, 15, 16, 17, 24, 30, 31, 57)
WIDTHS = (16, 32, 48, 64, 80, 128, 192, 256, 384, 768)


@pytest.fixture(scope="module")
def lib():
    from mrla_amd import _lib as L
    return L.load()


def test_token_part_rows_is_the_batch_size(lib):
    """The backward apply kernels are unbanded (token_bands_bwd): one row of partials per image at every side and width, also
    where the forward splits the map into 2 or 4 row bands, and for every element type."""
    from mrla_amd import _lib as L
    for side in SIDES:
        for c in WIDTHS:
            for b in (1, 2, 3, 128):
                for dt in (L.F32, L.BF16, L.F16):
                    assert lib.mrla_token_part_rows(b, 1 + side * side, c, dt) == b, (b, side, c, dt)


def test_token_part_rows_refuses_bad_arguments(lib):
    from mrla_amd import _lib as L
    assert lib.mrla_token_part_rows(2, 18, 64, L.F32) == L.EINVAL          # 17 map tokens: no square map
    assert lib.mrla_token_part_rows(2, 1, 64, L.F32) == L.EINVAL           # no map token at all
    assert lib.mrla_token_part_rows(0, 17, 64, L.F32) == L.EINVAL
    assert lib.mrla_token_part_rows(2, 17, 0, L.F32) == L.EINVAL
    assert lib.mrla_token_part_rows(2, 17, 64, 3) == L.EINVAL


@pytest.mark.parametrize("n", [2, 17, 197, 577])
def test_token_base_supported_widths(lib, n):
    """c % 64 == 0 and at most 256 16-byte vectors per pixel (base_nhwc_supported): every multiple of 64 up to 1024 in float32
    and up to 2048 in the 16-bit types -- DeiT's 192 / 384 / 768 are not powers of two."""
    from mrla_amd import _lib as L
    for b in (1, 3):
        for c in (64, 128, 192, 256, 384, 768, 1024):
            for dt in (L.F32, L.BF16, L.F16):
                assert lib.mrla_token_base_supported(b, n, c, dt) == 1, (b, c, dt)
        assert lib.mrla_token_base_supported(b, n, 2048, L.BF16) == 1
        assert lib.mrla_token_base_supported(b, n, 2048, L.F16) == 1
        assert lib.mrla_token_base_supported(b, n, 2048, L.F32) == 0
        for c in (32, 48, 96):
            for dt in (L.F32, L.BF16, L.F16):
                assert lib.mrla_token_base_supported(b, n, c, dt) == 0, (b, c, dt)


def test_token_base_supported_refuses_bad_arguments(lib):
    from mrla_amd import _lib as L
    assert lib.mrla_token_base_supported(2, 18, 64, L.F32) == L.EINVAL
    assert lib.mrla_token_base_supported(0, 197, 64, L.F32) == L.EINVAL
    assert lib.mrla_token_base_supported(2, 197, 64, 3) == L.EINVAL
    assert lib.mrla_token_base_supported(2, 197, 64, -1) == L.EINVAL


def test_rounding_reference_without_rounding_is_the_eager_module():
    """oracle.token_base_storage restates EagerTokenBaseModule (itself pinned to the reference's goldens) with rounding points;
    with the rounding off, a chain across a history reset gives the eager module's outputs and gradients in float64."""
    import numpy as np
    import torch
    from oracle import detgen, eager_models as em, token_base_storage as ts
    b, n, c, d, steps = 2, 10, 64, 16, 5

    def inputs(t):
        s = detgen.seed_of(f"tokbase-restated/{t}")
        return detgen.normalish((b, n, c), s).astype(np.float32), detgen.normalish((b, n, c), s + 1).astype(np.float32)

    def make(cls):
        def one(t):
            m = cls(c, d, init_cell=(t % 4 == 0))
            m.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.fill_state_dict(m.state_dict(), salt=70 + t).items()})
            return m
        return one
    got = ts.run_chain(make(ts.StorageTokenBaseModule), inputs, steps)
    want = ts.run_chain(make(em.EagerTokenBaseModule), inputs, steps)
    for t in range(steps):
        assert torch.allclose(got[2][t], want[2][t], rtol=0, atol=1e-13) and torch.allclose(got[3][t], want[3][t], rtol=0, atol=1e-13)
        assert torch.allclose(got[1][t].grad, want[1][t].grad, rtol=0, atol=1e-13)
        for (pn, p), (qn, q) in zip(got[0][t].named_parameters(), want[0][t].named_parameters()):
            assert pn == qn and torch.allclose(p.grad, q.grad, rtol=0, atol=1e-12), (t, pn)
    # and with it on, V_t, out and dx hold storage values only
    r = ts.run_chain(lambda t: make(lambda *a, **k: ts.StorageTokenBaseModule(*a, storage=torch.bfloat16, **k))(t), inputs, 2,
                     storage=torch.bfloat16)
    for v in (r[2][1], r[3][1], r[1][1].grad):
        assert torch.equal(v.to(torch.bfloat16).double(), v)
    assert not torch.equal(r[2][1], got[2][1])


def test_base_tile_rows_agrees_with_token_base_supported(lib):
    """The header documents mrla_base_tile_rows' widths as `c % 64 == 0 and c / (16 / sizeof(dtype)) <= 256`: the same predicate
    mrla_token_base_supported answers with, so the two never disagree on a multiple of 64."""
    from mrla_amd import _lib as L
    for c in range(64, 2048 + 1, 64):
        for dt, es in ((L.F32, 4), (L.BF16, 2), (L.F16, 2)):
            ok = c // (16 // es) <= 256
            rows = lib.mrla_base_tile_rows(2, c, 14, 14, dt, L.NHWC)
            assert (rows > 0) == ok and (ok or rows == L.EUNSUPPORTED), (c, dt, rows)
            assert lib.mrla_token_base_supported(2, 197, c, dt) == int(ok), (c, dt)
