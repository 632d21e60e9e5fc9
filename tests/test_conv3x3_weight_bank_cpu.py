"""Host side of mrla_conv3x3_weight_bank_refresh (mrla_amd/csrc/weight_bank.hip), of mrla_conv3x3_dgrad_flip_preferred
(mrla_amd/csrc/conv3x3_wgrad.hip) and of the switch functional.CONV3X3_DGRAD_FLIP.  Needs the built library, not a GPU.

  * both entry points are declared in include/mrla_hip.h, exported by the library and bound in _lib.SIGNATURES; the addition
    is additive (ABI 5, the signatures of the 1x1 bank as they were);
  * the refresh checks its arguments on the host: a NULL table, entries <= 0, max_tiles <= 0 and a dtype code that is none are
    MRLA_EINVAL, fp32 is MRLA_EUNSUPPORTED -- the codes of mrla_weight_bank_refresh_dt;
  * the rule refuses what mrla_conv3x3_wgrad_rows refuses at stride 1 with the same codes, answers 0 or 1 otherwise, 0 for
    fp16 (not measured), 0 where c != n, 0 for every 224 x 224 step up to batch 64 (the shapes the other test files run) and
    for the two small shapes of tests/launch_trace_cases.py, and is monotone in the batch;
  * the switch has its context manager, exported by the package, which restores on exit and on raise;
  * a call outside a model's bookkeeping, and a CPU tensor inside one, get conv(x) itself."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S1 = [(64, 56), (128, 28), (256, 14), (512, 7)]            # (channels, map) of the stride-1 3x3 convolutions of ResNet-50
REFRESH, RULE = "mrla_conv3x3_weight_bank_refresh", "mrla_conv3x3_dgrad_flip_preferred"


def test_the_entry_points_are_declared_exported_and_bound():
    from mrla_amd import _lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    assert re.search(rf"^int {REFRESH}\(const void\* table, int entries, int max_tiles, int dtype, void\* stream\);", header, re.M)
    assert re.search(rf"^int {RULE}\(int b, int c, int n, int h, int w, int dtype\);", header, re.M)
    assert L.SIGNATURES[REFRESH] == [L._P, L._I, L._I, L._I, L._P] and L.SIGNATURES[RULE] == [L._I] * 6
    assert hasattr(lib, REFRESH) and hasattr(lib, RULE)
    # additive: the version and the 1x1 bank's entry points are what they were
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and lib.mrla_abi_version() == 5
    assert L.SIGNATURES["mrla_weight_bank_refresh_dt"] == [L._P, L._I, L._I, L._I, L._P]
    assert L.SIGNATURES["mrla_weight_bank_refresh"] == [L._P, L._I, L._I, L._P]
    # exports still equal declarations
    declared = set(re.findall(r"^int (mrla_[a-z0-9_]+)\(", header, re.M))
    assert declared == set(L.SIGNATURES)


def test_the_refresh_checks_its_arguments_on_the_host():
    import ctypes
    from mrla_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_longlong * 5)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for dt in (L.BF16, L.F16):
        assert getattr(lib, REFRESH)(None, 1, 9, dt, None) == L.EINVAL
        assert getattr(lib, REFRESH)(p, 0, 9, dt, None) == L.EINVAL
        assert getattr(lib, REFRESH)(p, -1, 9, dt, None) == L.EINVAL
        assert getattr(lib, REFRESH)(p, 1, 0, dt, None) == L.EINVAL
    assert getattr(lib, REFRESH)(p, 1, 9, 7, None) == L.EINVAL
    assert getattr(lib, REFRESH)(p, 1, 9, -1, None) == L.EINVAL
    assert getattr(lib, REFRESH)(p, 1, 9, L.F32, None) == L.EUNSUPPORTED


def test_the_rule_refuses_what_rows_refuses_and_answers_0_or_1():
    from mrla_amd import _lib as L
    lib = L.load()
    rows, rule = lib.mrla_conv3x3_wgrad_rows, getattr(lib, RULE)
    for args in ((0, 512, 512, 7, 7), (8, 0, 512, 7, 7), (8, 512, -64, 7, 7), (8, 512, 512, 0, 7), (8, 512, 512, 7, -1)):
        for dt in (L.BF16, L.F16, L.F32, 7):
            assert rule(*args, dt) == rows(*args[:5], 1, dt) == L.EINVAL, (args, dt)
    good = (256, 512, 512, 7, 7)
    assert rule(*good, L.F32) == L.EUNSUPPORTED and rule(*good, 7) == L.EINVAL
    for b in (1, 8, 32, 64, 128, 256, 1024):
        for c, hw in S1:
            assert rule(b, c, c, hw, hw, L.BF16) in (0, 1)
            assert rule(b, c, c, hw, hw, L.F16) == 0                        # fp16 was not measured: bf16 alone is routed
            assert rule(b, c, 2 * c, hw, hw, L.BF16) == 0 and rule(b, 2 * c, c, hw, hw, L.BF16) == 0      # c == n only
    assert rule(2 ** 31 - 1, 64, 64, 2 ** 31 - 1, 2 ** 31 - 1, L.BF16) in (0, 1)        # no overflow in the rule's product


def test_the_shapes_the_other_test_files_run_stay_on_the_stock_operator():
    from mrla_amd import _lib as L
    rule = getattr(L.load(), RULE)
    for shape in ((2, 64, 64, 16, 16), (8, 64, 64, 16, 16), (64, 512, 512, 7, 7), (5, 64, 64, 28, 28)):
        assert rule(*shape, L.BF16) == 0, shape
    for b in (1, 2, 4, 8, 16, 32, 64):                                      # whole-model steps on 224 x 224 images
        for c, hw in S1:
            assert rule(b, c, c, hw, hw, L.BF16) == 0, (b, c, hw)
    for c, h, w in ((64, 48, 80), (128, 24, 40), (256, 12, 20), (512, 6, 10), (64, 24, 24), (64, 16, 16)):
        assert rule(16, c, c, h, w, L.BF16) == 0, (c, h, w)                 # the detection and 64 / 96-pixel model tests


def test_the_rule_is_monotone_in_the_batch_and_routes_the_large_batch_step():
    from mrla_amd import _lib as L
    rule = getattr(L.load(), RULE)
    for c, hw in S1:
        answers = [rule(b, c, c, hw, hw, L.BF16) for b in range(1, 513)]
        assert answers == sorted(answers), (c, hw)                          # 0 ... 0 1 ... 1
        assert answers[-1] == 1 and answers[255] == 1, (c, hw)              # the flagship step (batch 256) is routed


def test_the_switch_has_a_context_manager_that_restores():
    import mrla_amd
    from mrla_amd import functional as F
    before = F.CONV3X3_DGRAD_FLIP
    assert mrla_amd.conv3x3_dgrad_flip is F.conv3x3_dgrad_flip
    for value in (True, False):
        with mrla_amd.conv3x3_dgrad_flip(value):
            assert F.CONV3X3_DGRAD_FLIP is value
            with mrla_amd.conv3x3_dgrad_flip(not value):
                assert F.CONV3X3_DGRAD_FLIP is (not value)
            assert F.CONV3X3_DGRAD_FLIP is value
        assert F.CONV3X3_DGRAD_FLIP is before
    with pytest.raises(KeyError):
        with mrla_amd.conv3x3_dgrad_flip(not before):
            raise KeyError("x")
    assert F.CONV3X3_DGRAD_FLIP is before
    # the siblings are left alone
    with mrla_amd.conv3x3_dgrad_flip(not before):
        assert (F.CONV3X3_WGRAD, F.CONV3X3_WGRAD_AUTO, F.CONV3X3_FWD, F.CONV3X3_DGRAD) == (False, True, False, False)


def test_without_a_bank_and_on_the_cpu_it_is_conv_itself():
    from mrla_amd import functional as F
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False)
    x = torch.randn(2, 64, 5, 5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bank = F.Conv3x3Bank()
    with F.conv3x3_dgrad_flip(True):
        y0 = F.conv3x3(x, conv)                                             # no bookkeeping scope
        with F.batched_bookkeeping(0, None, bank):
            y1 = F.conv3x3(x, conv)                                         # a CPU tensor inside one
    for y in (y0, y1):
        assert type(y.grad_fn).__name__ == "ConvolutionBackward0" and torch.equal(y, conv(x))
    assert bank.members == [] and bank.entries == {} and bank.table is None
    assert F.Conv3x3Bank.eligible(conv) is False                            # a CPU weight
