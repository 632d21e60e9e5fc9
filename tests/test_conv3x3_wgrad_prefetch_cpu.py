"""Host side of mrla_conv3x3_wgrad_preferred (mrla_amd/csrc/conv3x3_wgrad.hip) and of the route by shape in the Python layer
(functional.CONV3X3_WGRAD_AUTO, mrla_amd.conv3x3_wgrad_auto()).  Needs the built library, not a GPU.

  * the query is exported, declared and bound, and refuses what mrla_conv3x3_wgrad_rows refuses, with the same codes;
  * it answers 0 at the batch 8 / 16 shapes, where the own kernel loses, and at every stride-2 convolution of ResNet-50, and 1
    at the classes profiles/conv3x3_wgrad.md section 7 found to win: the stride-1 convolutions of ResNet-50 at batch 64, 128
    and 256 (392 output pixels per split or more; level at batch 32, 196 - 224 pixels, which stays 0);
  * the switch is on by default, restores on exit and on raise, and leaves CONV3X3_WGRAD and reproducible_gradients() alone;
  * with it on, a CPU tensor and every excluded configuration still get conv(x) itself."""
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
