"""CPU-only checks of the row-band geometry of the fused stem tail (mrla_bn_relu_pool_*; mrla_amd/csrc/stem_pool_nhwc.hip) as
mrla_bn_pool_plan reports it -- the same function the kernels' prologue takes a band's window rows from.  The backward kernel
always runs a band's last one or two steps: a band without a window row stores rows that are not its own (the next image's, or
past the tensor).  So over a sweep of shapes: the bands tile [0, Ho) in order and NONE IS EMPTY, their number is a power of two
<= 32 that divides the pixel count (the statistics pass's (rows, count) form), and mrla_bn_pool_rows counts b * bands rows."""
import ctypes

import pytest

HS = range(2, 301)
WS = (2, 3, 4, 5, 8, 16, 32, 112, 672)
BCS = ((1, 64), (2, 64), (2, 128), (8, 64), (256, 64))
EXPLICIT = ((2, 64, 400, 672), (256, 64, 112, 112))

# (b, c, h, w) -> row bands per image.  Pinned so that a change of pool_geo's heuristic is a visible decision: the first six
# are shapes where the ceil(Ho / bands) split this partition replaced left 1 .. 6 trailing bands empty.
PINNED_BANDS = {(1, 64, 66, 4): 8, (1, 64, 65, 8): 8, (1, 64, 70, 4): 8, (1, 64, 82, 4): 8, (1, 64, 258, 32): 32,
                (2, 64, 400, 672): 32, (4, 64, 112, 112): 8, (1, 192, 30, 34): 2}


def _plan(lib, L, shape, band, dtype=None):
    out = (ctypes.c_int * 6)()
    rc = lib.mrla_bn_pool_plan(*shape, L.BF16 if dtype is None else dtype, L.NHWC, band, ctypes.cast(out, ctypes.c_void_p))
    assert rc == L.OK, (shape, band, rc)
    return tuple(out)


def _check(lib, L, shape):
    b, c, h, w = shape
    ho, wo, bands, waves, lo, hi = _plan(lib, L, shape, 0)
    assert (ho, wo) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1), shape
    assert lib.mrla_bn_pool_rows(b, c, h, w, L.BF16, L.NHWC) == b * bands, shape
    assert 1 <= bands <= 32 and bands & (bands - 1) == 0, (shape, bands)
    assert (h * w) % bands == 0, (shape, bands)
    assert 1 <= waves <= 8 and waves == min(8, (wo + 3) // 4), (shape, waves)
    edge = 0
    for band in range(bands):
        p = _plan(lib, L, shape, band)
        assert p[:4] == (ho, wo, bands, waves), (shape, band)
        assert p[4] == edge, (shape, band, p)                   # contiguous from 0 ...
        assert p[5] > p[4], (shape, band, p)                    # ... and not empty
        edge = p[5]
    assert edge == ho, (shape, edge)                            # ... up to Ho
    return bands


@pytest.mark.parametrize("bc", BCS, ids=lambda bc: "x".join(map(str, bc)))
def test_every_row_band_is_a_nonempty_piece_of_a_partition(bc):
    from mrla_amd import _lib as L
    lib = L.load()
    for h in HS:
        for w in WS:
            _check(lib, L, (*bc, h, w))


def test_explicit_and_pinned_shapes():
    from mrla_amd import _lib as L
    lib = L.load()
    for shape in EXPLICIT:
        _check(lib, L, shape)
    for shape, bands in PINNED_BANDS.items():
        assert _check(lib, L, shape) == bands, shape
        # the geometry does not depend on the element type, and the Python helper answers the same
        for dt in (L.F32, L.BF16, L.F16):
            assert _plan(lib, L, shape, bands - 1, dt) == _plan(lib, L, shape, bands - 1) == L.bn_pool_plan(*shape, dt, bands - 1)
    # where bands divides Ho the pieces are the equal ones the 224-pixel stem has always had
    assert [_plan(lib, L, (4, 64, 112, 112), i)[4:] for i in range(8)] == [(7 * i, 7 * i + 7) for i in range(8)]
    # uneven: the remainder is spread, no piece differs from another by more than one row
    sizes = [hi - lo for lo, hi in (_plan(lib, L, (2, 64, 400, 672), i)[4:] for i in range(32))]
    assert sum(sizes) == 200 and set(sizes) == {6, 7}
