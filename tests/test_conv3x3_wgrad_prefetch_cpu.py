"""Host side of mrla_conv3x3_wgrad_preferred (mrla_amd/csrc/conv3x3_wgrad.hip) and of the route by shape in the Python layer
(functional.CONV3X3_WGRAD_AUTO, mrla_amd.conv3x3_wgrad_auto()).  Needs the built library, not a GPU.

  * the query is exported, declared and bound, and refuses what mrla_conv3x3_wgrad_rows refuses, with the same codes;
  * it answers 0 at the batch 8 / 16 shapes, where the own kernel loses, and at every stride-2 convolution of ResNet-50, and 1
    at the classes profiles/conv3x3_wgrad.md section 7 found to win: the stride-1 convolutions of ResNet-50 at batch 64, 128
    and 256 (392 output pixels per split or more; level at batch 32, 196 - 224 pixels, which stays 0);
  * the switch is on by default, restores on exit and on raise, and leaves CONV3X3_WGRAD and reproducible_gradients() alone;
  * with it on, a CPU tensor and every excluded configuration still get conv(x) itself;
  * the threshold either side of its flip at five shape classes, and over a grid of shapes the query recomputed from the plan's
    rows per split and the documented rule;
  * the matmul form of the float64 reference that tests/test_conv3x3_wgrad_auto_gpu.py uses, held equal to the autograd form."""
import os
import re

import pytest
import torch

from tests.test_conv3x3_wgrad_cpu import _conv, excluded_configurations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S1 = [(64, 56), (128, 28), (256, 14), (512, 7)]            # (channels, map) of the stride-1 3x3 convolutions of ResNet-50
S2 = [(128, 56), (256, 28), (512, 14)]                     # ... of the stride-2 ones
WINNING_BATCHES = (64, 128, 256)                           # profiles/conv3x3_wgrad.md section 7: every stride-1 shape wins at these


def test_the_query_is_exported_declared_and_bound():
    from mrla_amd import _lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    name = "mrla_conv3x3_wgrad_preferred"
    assert hasattr(lib, name) and L.SIGNATURES[name] == L.SIGNATURES["mrla_conv3x3_wgrad_rows"]
    assert re.search(rf"^int {name}\(", header, re.M)
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and lib.mrla_abi_version() == 5


def test_the_query_refuses_what_rows_refuses_with_the_same_codes():
    from mrla_amd import _lib as L
    lib = L.load()
    rows, pref = lib.mrla_conv3x3_wgrad_rows, lib.mrla_conv3x3_wgrad_preferred
    cases = [(8, 96, 512, 7, 7, 1), (8, 512, 96, 7, 7, 1), (8, 512, 512, 7, 7, 3), (8, 512, 512, 7, 7, 4),
             (256, 64, 64, 256, 256, 1), (64, 64, 256, 256, 256, 2),
             (0, 512, 512, 7, 7, 1), (8, 0, 512, 7, 7, 1), (8, 512, -64, 7, 7, 1), (8, 512, 512, 0, 7, 1), (8, 512, 512, 7, -1, 1),
             (8, 512, 512, 7, 7, 0)]
    for args in cases:
        for dt in (L.BF16, L.F16, L.F32, 7):
            assert rows(*args, dt) < 0 and pref(*args, dt) == rows(*args, dt), (args, dt)
    good = (256, 512, 512, 7, 7, 1)
    assert pref(*good, L.F32) == rows(*good, L.F32) == L.EUNSUPPORTED and pref(*good, 7) == rows(*good, 7) == L.EINVAL
    # every accepted shape gets 0 or 1, the same for both 16-bit types
    for b in (1, 8, 64, 256):
        for c, hw in S1 + S2:
            for s in (1, 2):
                assert rows(b, c, c, hw, hw, s, L.BF16) > 0
                assert pref(b, c, c, hw, hw, s, L.BF16) == pref(b, c, c, hw, hw, s, L.F16) in (0, 1)
    assert pref(255, 64, 64, 256, 256, 1, L.BF16) in (0, 1)                  # just below the size bound


def test_small_batches_and_stride_2_stay_on_the_stock_operator():
    from mrla_amd import _lib as L
    pref = L.load().mrla_conv3x3_wgrad_preferred
    for shape in ((8, 512, 512, 7, 7, 1), (16, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2), (16, 512, 512, 14, 14, 2)):
        assert pref(*shape, L.BF16) == 0 and pref(*shape, L.F16) == 0, shape
    for b in (8, 16, 32, 64, 128, 256):
        for c, hw in S2:
            assert pref(b, c, c, hw, hw, 2, L.BF16) == 0, (b, c, hw)         # no stride-2 class measurably won
        for c, hw in S1:
            if b <= 32:
                assert pref(b, c, c, hw, hw, 1, L.BF16) == 0, (b, c, hw)


def test_the_classes_the_profile_found_to_win_are_preferred():
    from mrla_amd import _lib as L
    pref = L.load().mrla_conv3x3_wgrad_preferred
    for b in WINNING_BATCHES:
        for c, hw in S1:
            assert pref(b, c, c, hw, hw, 1, L.BF16) == 1 and pref(b, c, c, hw, hw, 1, L.F16) == 1, (b, c, hw)


def test_the_switch_is_on_by_default_and_leaves_the_other_switches_alone():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_WGRAD_AUTO is True and Fm.CONV3X3_WGRAD is False and Fm.STEM_WGRAD is False
    with mrla_amd.conv3x3_wgrad_auto(False):
        assert Fm.CONV3X3_WGRAD_AUTO is False and Fm.CONV3X3_WGRAD is False
        with mrla_amd.conv3x3_wgrad_auto():
            assert Fm.CONV3X3_WGRAD_AUTO is True
        assert Fm.CONV3X3_WGRAD_AUTO is False
    assert Fm.CONV3X3_WGRAD_AUTO is True
    with pytest.raises(RuntimeError):
        with mrla_amd.conv3x3_wgrad_auto(False):
            raise RuntimeError("x")
    assert Fm.CONV3X3_WGRAD_AUTO is True                         # the previous value comes back when the block raises
    with mrla_amd.conv3x3_wgrad():
        assert Fm.CONV3X3_WGRAD is True and Fm.CONV3X3_WGRAD_AUTO is True
    with mrla_amd.reproducible_gradients():
        assert Fm.CONV3X3_WGRAD is True and Fm.STEM_WGRAD is True and Fm.CONV3X3_WGRAD_AUTO is True
    with mrla_amd.conv3x3_wgrad_auto(False), mrla_amd.reproducible_gradients():
        assert Fm.CONV3X3_WGRAD is True and Fm.STEM_WGRAD is True and Fm.CONV3X3_WGRAD_AUTO is False
    assert (Fm.CONV3X3_WGRAD_AUTO, Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (True, False, False)


def test_with_the_switch_on_ineligible_calls_get_the_module_itself():
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_WGRAD_AUTO is True
    conv = _conv()
    x = torch.randn(2, 64, 5, 5, requires_grad=True)
    y = Fm.conv3x3(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn).__name__ == type(conv(x).grad_fn).__name__
    for name, c, make in excluded_configurations():
        xin = make("cpu").requires_grad_(True)
        c = c.to(xin.dtype)
        assert not Fm._conv3x3_own_wgrad(c, xin), name
        y = Fm.conv3x3(xin, c)
        assert type(y.grad_fn).__name__ == type(c(xin).grad_fn).__name__ and torch.equal(y, c(xin)), name


# (channels in, channels out, h, w, the batch one below the flip: answers 0, the batch at the flip: answers 1), both 16-bit types.
# By c3_plan's arithmetic: tiles = (n / 64) * (c / 64), want = ceil(512 / tiles) splits, per = ceil(b * h / want) rows per
# split, and the rule needs per * w >= 384 and ceil(per / rmax) * nseg >= 4.  512 -> 512 on 7 x 7: 64 tiles, 8 splits, so
# per >= 55 (385 pixels) needs b * 7 > 54 * 8 = 432 rows: batch 62 (434 rows); batch 61 has 427 rows, 54 a split, 378 pixels.
THRESHOLDS = [
    (512, 512, 7, 7, 61, 62),
    (256, 256, 14, 14, 61, 62),
    (128, 128, 28, 28, 59, 60),
    (64, 64, 56, 56, 54, 55),
    (64, 256, 6, 131, 42, 43),
]
GRID_CHANNELS = (64, 128, 256, 512)
GRID_MAPS = ((7, 7), (14, 14), (28, 28), (56, 56), (6, 131))


def test_the_threshold_sits_where_the_planners_arithmetic_puts_it():
    from mrla_amd import _lib as L
    pref = L.load().mrla_conv3x3_wgrad_preferred
    for c, n, h, w, below, at in THRESHOLDS:
        assert at == below + 1
        for dt in (L.BF16, L.F16):
            assert pref(below, c, n, h, w, 1, dt) == 0 and pref(at, c, n, h, w, 1, dt) == 1, (c, n, h, w)
            assert all(pref(b, c, n, h, w, 1, dt) == 0 for b in range(1, below)), (c, n, h, w)       # ... and it is THE flip
            assert all(pref(b, c, n, h, w, 1, dt) == 1 for b in range(at, 81)), (c, n, h, w)
    # 512 -> 512 on 7 x 7 at batch 55 and 56: 385 and 392 rows over 8 splits are 49 rows per split, 343 pixels -- below 384, both
    # answer 0 (56 ROWS per split, 392 pixels, is what batch 63 and 64 have)
    for b, rows in ((55, 49), (56, 49), (61, 54), (62, 55), (63, 56), (64, 56)):
        assert L.conv3x3_wgrad_plan(b, 512, 512, 7, 7, 1, L.BF16)[2] == rows, b
        assert pref(b, 512, 512, 7, 7, 1, L.BF16) == pref(b, 512, 512, 7, 7, 1, L.F16) == int(rows * 7 >= 384), b
    # four steps, but 16 splits of 28 rows: 196 pixels
    for shape in ((64, 256, 512, 7, 7, 1), (64, 512, 256, 7, 7, 1)):
        plan = L.conv3x3_wgrad_plan(*shape, L.BF16)
        assert plan[2] == 28 and plan[4] == 16 and -(-plan[2] // 7) == 4
        assert pref(*shape, L.BF16) == 0 and pref(*shape, L.F16) == 0, shape


def test_the_query_is_the_documented_rule_on_the_plans_rows_per_split():
    """Every accepted stride-1 shape of a modest grid: ceil(per / rmax) * nseg >= 4 and per * wo >= 384 (conv3x3_wgrad.hip:
    kC3PreferSteps, kC3PreferPixels), `per` from mrla_conv3x3_wgrad_plan, rmax and nseg by conv_spatial.h's raster rule (whole
    rows while the pitch wo + 2 is at most 60 and as many of them as 128 raster pixels hold, else one row in segments of 58)."""
    from mrla_amd import _lib as L
    pref = L.load().mrla_conv3x3_wgrad_preferred
    ones = 0
    for h, w in GRID_MAPS:
        rmax, nseg = (max(1, min(h, 128 // (w + 2))), 1) if w + 2 <= 60 else (1, -(-w // 58))
        for c in GRID_CHANNELS:
            for n in GRID_CHANNELS:
                for b in range(1, 81):
                    plan = L.conv3x3_wgrad_plan(b, c, n, h, w, 1, L.BF16)
                    assert plan is not None, (b, c, n, h, w)
                    want = int(-(-plan[2] // rmax) * nseg >= 4 and plan[2] * w >= 384)
                    assert pref(b, c, n, h, w, 1, L.BF16) == pref(b, c, n, h, w, 1, L.F16) == want, (b, c, n, h, w)
                    assert pref(b, c, n, 2 * h, 2 * w, 2, L.BF16) == 0
                    ones += want
    assert 0 < ones < 80 * 16 * 5                            # (the grid has both answers)


def test_the_matmul_reference_equals_the_autograd_reference():
    """_dw64_taps of tests/test_conv3x3_wgrad_auto_gpu.py (nine float64 matmuls) against _dw64 of tests/test_conv3x3_wgrad_gpu.py
    (float64 autograd of F.conv2d) at two small shapes of each stride: equal on the dyadic inputs, where every float64 sum is
    exact; on normal inputs within the two float64 summation errors, 2 * P * 2^-53 * A, P pixels in the sum."""
    from tests.test_conv3x3_wgrad_auto_gpu import _dw64_taps
    from tests.test_conv3x3_wgrad_gpu import _dw64, _inputs
    for shape in ((2, 64, 128, 7, 7, 1), (3, 128, 64, 8, 33, 1), (2, 64, 64, 9, 6, 2), (1, 64, 64, 3, 131, 2)):
        s = shape[5]
        x, dy = _inputs(shape, "dyadic")
        assert torch.equal(_dw64_taps(x, dy, s), _dw64(x, dy, s)), shape
        x, dy = _inputs(shape, "normal", "bf16")
        got, want, a = _dw64_taps(x, dy, s), _dw64(x, dy, s), _dw64(x.abs(), dy.abs(), s)
        pixels = dy.numel() // dy.shape[1]
        assert got.shape == want.shape and bool(((got - want).abs() <= 2 * pixels * 2.0 ** -53 * a).all()), shape
        assert float(want.abs().max()) > 0
