"""Host side and compiler side of mrla_conv3x3_fwd (mrla_amd/csrc/conv3x3_fwd.hip) and of its switch in the Python layer.
Needs the built library and, for the resource figures, hipcc -- not a GPU.

  * the three symbols are exported, declared and bound, the ABI version is still 5;
  * argument validation: every MRLA_EINVAL / MRLA_EUNSUPPORTED case of the header's contract, decided before any launch, and
    the queries answering the launch's codes;
  * the planner: record rows = the plan's, and the workgroups' ranges of output rows tile all output rows exactly once;
  * no scratch in any of the eight compiled instances;
  * the switch is off by default, off means conv(x) itself, it nests and comes back when the block raises;
    conv3x3_fwd_applies refuses CPU tensors and every excluded configuration but the frozen weight, which it takes;
    conv3x3_bn_act with the switch off is bn_act(conv3x3(...))."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.test_conv3x3_wgrad_cpu import WIDTHS, _conv, excluded_configurations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402


def test_symbols_are_exported_and_declared():
    from mrla_amd import _lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    for name in ("mrla_conv3x3_fwd_rows", "mrla_conv3x3_fwd_plan", "mrla_conv3x3_fwd"):
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert L.SIGNATURES["mrla_conv3x3_fwd"] == [L._P] * 4 + [L._I] * 7 + [L._P]
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5


def test_queries_validate_their_arguments():
    from mrla_amd import _lib as L
    lib = L.load()
    rows, plan = lib.mrla_conv3x3_fwd_rows, lib.mrla_conv3x3_fwd_plan
    out = (ctypes.c_int * 6)()
    po = ctypes.cast(out, ctypes.c_void_p)
    good = (8, 512, 512, 7, 7, 1)
    for dt in (L.BF16, L.F16):
        assert rows(*good, dt) > 0 and plan(*good, dt, po) == L.OK and out[4] == rows(*good, dt)
    cases = [((8, 96, 512, 7, 7, 1), L.EUNSUPPORTED), ((8, 512, 96, 7, 7, 1), L.EUNSUPPORTED),     # c, n % 64
             ((8, 512, 512, 7, 7, 3), L.EUNSUPPORTED), ((8, 512, 512, 7, 7, 4), L.EUNSUPPORTED),   # other strides
             ((256, 64, 64, 256, 256, 1), L.EUNSUPPORTED), ((64, 64, 256, 256, 256, 2), L.EUNSUPPORTED),      # b*h*w*max(c,n)*2 = 2^31
             ((0, 512, 512, 7, 7, 1), L.EINVAL), ((8, 0, 512, 7, 7, 1), L.EINVAL), ((8, 512, -64, 7, 7, 1), L.EINVAL),
             ((8, 512, 512, 0, 7, 1), L.EINVAL), ((8, 512, 512, 7, -1, 1), L.EINVAL), ((8, 512, 512, 7, 7, 0), L.EINVAL)]
    for args, code in cases:
        for dt in (L.BF16, L.F16):
            assert rows(*args, dt) == code, (args, dt)
            assert plan(*args, dt, po) == code, (args, dt)
    assert rows(255, 64, 64, 256, 256, 1, L.BF16) > 0                        # just below the bound
    assert rows(*good, L.F32) == L.EUNSUPPORTED and plan(*good, L.F32, po) == L.EUNSUPPORTED
    assert rows(*good, 7) == L.EINVAL and plan(*good, 7, po) == L.EINVAL     # a dtype code that is none
    assert plan(*good, L.BF16, None) == L.EINVAL                             # null out


def test_launch_validates_its_arguments_before_launching():
    from mrla_amd import _lib as L
    lib = L.load()
    one, two, three, four = (ctypes.c_void_p(16 * i) for i in (1, 2, 3, 4))
    odd = ctypes.c_void_p(24)

    def call(dtype, shape=(8, 512, 512, 7, 7, 1), x=one, wt=two, y=three, mom=four):
        return lib.mrla_conv3x3_fwd(x, wt, y, mom, *shape, dtype, None)
    # nothing is launched in any of these
    for name in ("x", "wt", "y"):
        assert call(L.BF16, **{name: None}) == L.EINVAL, name
        assert call(L.BF16, **{name: odd}) == L.EINVAL, name
        assert call(L.F16, **{name: odd}) == L.EINVAL, name
        assert call(L.BF16, mom=None, **{name: odd}) == L.EINVAL, name
    assert call(L.BF16, mom=odd) == L.EINVAL and call(L.F16, mom=odd) == L.EINVAL        # (a NULL mom_part is no records)
    assert call(7) == L.EINVAL
    assert call(L.F32) == L.EUNSUPPORTED and call(L.F32, mom=None) == L.EUNSUPPORTED
    for shape in ((8, 96, 512, 7, 7, 1), (8, 512, 96, 7, 7, 1), (8, 512, 512, 7, 7, 3), (256, 64, 64, 256, 256, 1)):
        assert call(L.BF16, shape=shape) == L.EUNSUPPORTED, shape
        assert call(L.F16, shape=shape, mom=None) == L.EUNSUPPORTED, shape
    for shape in ((0, 512, 512, 7, 7, 1), (8, 512, 512, 7, 0, 1), (8, 512, 512, 7, 7, 0), (8, -64, 512, 7, 7, 1)):
        assert call(L.BF16, shape=shape) == L.EINVAL, shape


def test_rows_equal_the_plans_record_rows():
    from mrla_amd import _lib as L
    lib = L.load()
    for b, c, n, h, w, s in ((1, 64, 64, 1, 1, 1), (2, 64, 128, 7, 7, 1), (3, 128, 64, 8, 33, 1), (256, 64, 64, 56, 56, 1),
                             (256, 128, 128, 56, 56, 2), (256, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2), (1, 64, 64, 1, 4000, 2),
                             (16, 256, 256, 14, 14, 1), (2, 576, 64, 9, 6, 2)):
        for dt in (L.BF16, L.F16):
            plan = L.conv3x3_fwd_plan(b, c, n, h, w, s, dt)
            assert plan is not None and plan[4] == lib.mrla_conv3x3_fwd_rows(b, c, n, h, w, s, dt) > 0, (b, c, n, h, w, s)
    assert L.conv3x3_fwd_plan(2, 96, 64, 7, 7, 1) is None


def test_the_ranges_tile_the_output_rows_exactly_once():
    """b in {1, 2, 8, 256}, the four ResNet widths, maps 1 .. 57, both strides.  Range i takes the output rows
    [i * per, min(total, (i + 1) * per)): together every row once, none empty; a step holds whole rows or one segment; at most
    256 workgroups, and `per` is at least a step's rows (the last range takes the remainder)."""
    from mrla_amd import _lib as L
    for b in (1, 2, 8, 256):
        for width in WIDTHS:
            for hw in range(1, 58):
                for s in (1, 2):
                    tn, per, rstep, nseg, rows, wgs = L.conv3x3_fwd_plan(b, width, width, hw, hw, s, L.BF16)
                    total = b * ((hw - 1) // s + 1)
                    assert per >= 1 and rows >= 1 and rstep >= 1 and nseg >= 1 and (nseg == 1 or rstep == 1)
                    assert width % tn == 0 and wgs == rows * (width // tn)
                    assert (rows - 1) * per < total <= rows * per, (b, width, hw, s, per, rows)      # no gap, no empty range
                    assert rows <= -(-256 // (width // tn)), (b, width, hw, s, rows)      # at most one workgroup per CU
                    # a range is at least a full step (two where c = 64, whose weights are loaded once), unless it is the only one
                    assert rows == 1 or per >= (2 if width == 64 else 1) * rstep, (b, width, hw, s, per, rstep)


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_of_the_new_file_uses_scratch():
    kernels = kr.kernel_resources("conv3x3_fwd.hip")
    main = [k for k in kernels if "conv3x3_fwd_kernel" in k["mangled"]]
    assert len(main) == 8 and len(kernels) == 8               # bf16 / fp16 x stride 1 / 2 x with / without records
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"instances with scratch (bytes per lane): {bad}"
    for k in main:
        assert k["waves"] >= 1, (k["mangled"], k["vgprs"], k["agprs"])


def test_the_switch_is_off_by_default_and_off_means_the_module_itself():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_FWD is False
    conv = _conv()
    x = torch.randn(2, 64, 5, 5, requires_grad=True)
    y = Fm.conv3x3(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
    with mrla_amd.conv3x3_fwd():
        assert Fm.CONV3X3_FWD is True
        with mrla_amd.conv3x3_fwd(False):
            assert Fm.CONV3X3_FWD is False
        assert Fm.CONV3X3_FWD is True
        y = Fm.conv3x3(x, conv)                                    # a CPU tensor: not eligible, the module itself
        assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
    assert Fm.CONV3X3_FWD is False
    with pytest.raises(RuntimeError):
        with mrla_amd.conv3x3_fwd():
            raise RuntimeError("x")
    assert Fm.CONV3X3_FWD is False                               # the previous value comes back when the block raises
    with mrla_amd.reproducible_gradients():                      # ... which leaves this switch alone
        assert Fm.CONV3X3_FWD is False


def test_applies_is_false_for_cpu_tensors_and_every_excluded_configuration_but_the_frozen_weight(monkeypatch):
    from mrla_amd import functional as Fm
    conv = _conv().bfloat16()
    x = torch.randn(2, 64, 6, 6).bfloat16().contiguous(memory_format=torch.channels_last)
    assert not Fm.conv3x3_fwd_applies(conv, x)
    names = []
    for name, c, make in excluded_configurations():
        assert not Fm.conv3x3_fwd_applies(c.bfloat16(), make("cpu")), name
        names.append(name)
    assert "frozen weight" in names

    # apart from the device check the frozen weight is eligible, also under no_grad, and the others are not: the same
    # tensors claiming to be CUDA tensors (no GPU here; is_cuda is all the check reads of the device)
    class _OnDevice(torch.Tensor):
        is_cuda = True

    def claim(t):
        return t.as_subclass(_OnDevice)
    for name, c, make in excluded_configurations():
        c = c.bfloat16()
        c.weight = torch.nn.Parameter(claim(c.weight.data), requires_grad=c.weight.requires_grad)
        got = Fm.conv3x3_fwd_applies(c, claim(make("cpu")))
        assert got == (name == "frozen weight"), name
        if name == "frozen weight":
            with torch.no_grad():
                assert Fm.conv3x3_fwd_applies(c, claim(make("cpu")))
            assert not Fm.conv3x3_applies(c, claim(make("cpu")))     # (the weight-gradient route still refuses it)


def test_conv_bn_act_with_the_switch_off_is_bn_act_of_conv3x3():
    from mrla_amd import functional as Fm
    torch.manual_seed(3)
    conv, bn = _conv(), torch.nn.BatchNorm2d(64)
    x = torch.randn(2, 64, 5, 5)
    for relu in (True, False):
        for train in (True, False):
            bn.train(train)
            bn2 = torch.nn.BatchNorm2d(64).train(train)
            bn2.load_state_dict(bn.state_dict())
            got = Fm.conv3x3_bn_act(x, conv, bn, relu)
            want = Fm.bn_act(Fm.conv3x3(x, conv), bn2, relu)
            assert torch.equal(got, want) and type(got.grad_fn) is type(want.grad_fn)
            assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var)
