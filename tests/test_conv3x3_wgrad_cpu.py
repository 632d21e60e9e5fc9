"""Host side and compiler side of mrla_conv3x3_wgrad (mrla_amd/csrc/conv3x3_wgrad.hip) and of its switch in the Python layer.
Needs the built library and, for the resource figures, hipcc -- not a GPU.

  * argument validation: every MRLA_EINVAL / MRLA_EUNSUPPORTED case of the header's contract, decided before any launch, and
    the queries answering the launch's codes;
  * the planner: splits = rows of part, and the splits' ranges of output rows tile all output rows exactly once, none empty;
  * no scratch in any compiled instance (the accumulators of nine taps are 144 registers of a lane);
  * the switch is off by default, and off means conv(x) itself; conv3x3_applies refuses CPU tensors and every excluded
    configuration."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

WIDTHS = (64, 128, 256, 512)


def test_symbols_are_exported_and_declared():
    from mrla_amd import _lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    for name in ("mrla_conv3x3_wgrad_rows", "mrla_conv3x3_wgrad_plan", "mrla_conv3x3_wgrad"):
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5


def test_queries_validate_their_arguments():
    from mrla_amd import _lib as L
    lib = L.load()
    rows, plan = lib.mrla_conv3x3_wgrad_rows, lib.mrla_conv3x3_wgrad_plan
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

    def call(dtype, dw_dtype, shape=(8, 512, 512, 7, 7, 1), dy=one, x=two, part=three, dw=four):
        return lib.mrla_conv3x3_wgrad(dy, x, part, dw, *shape, dtype, dw_dtype, None)
    # nothing is launched in any of these
    for name in ("dy", "x", "part", "dw"):
        assert call(L.BF16, L.F32, **{name: None}) == L.EINVAL, name
        assert call(L.BF16, L.F32, **{name: odd}) == L.EINVAL, name
        assert call(L.F16, L.F16, **{name: odd}) == L.EINVAL, name
    assert call(L.BF16, L.F16) == L.EINVAL and call(L.F16, L.BF16) == L.EINVAL      # a 16-bit dw_dtype other than dtype
    assert call(L.BF16, 7) == L.EINVAL and call(7, L.F32) == L.EINVAL
    assert call(L.F32, L.F32) == L.EUNSUPPORTED
    for shape in ((8, 96, 512, 7, 7, 1), (8, 512, 512, 7, 7, 3), (256, 64, 64, 256, 256, 1)):
        assert call(L.BF16, L.F32, shape=shape) == L.EUNSUPPORTED, shape
        assert call(L.F16, L.F16, shape=shape) == L.EUNSUPPORTED, shape
    for shape in ((0, 512, 512, 7, 7, 1), (8, 512, 512, 7, 0, 1), (8, 512, 512, 7, 7, 0), (8, -64, 512, 7, 7, 1)):
        assert call(L.BF16, L.F32, shape=shape) == L.EINVAL, shape


def test_rows_equal_the_plans_splits():
    from mrla_amd import _lib as L
    lib = L.load()
    for b, c, n, h, w, s in ((1, 64, 64, 1, 1, 1), (2, 64, 128, 7, 7, 1), (3, 128, 64, 8, 33, 1), (256, 64, 64, 56, 56, 1),
                             (256, 128, 128, 56, 56, 2), (256, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2), (1, 64, 64, 1, 4000, 2),
                             (16, 256, 256, 14, 14, 1), (2, 576, 64, 9, 6, 2)):
        for dt in (L.BF16, L.F16):
            plan = L.conv3x3_wgrad_plan(b, c, n, h, w, s, dt)
            assert plan is not None and plan[4] == lib.mrla_conv3x3_wgrad_rows(b, c, n, h, w, s, dt) > 0, (b, c, n, h, w, s)


def test_the_splits_tile_the_output_rows_exactly_once():
    """b in {1, 2, 8, 256}, the four ResNet widths, maps 1 .. 57, both strides.  Split i takes the output rows
    [i * per, min(total, (i + 1) * per)): together every row once, none empty; tiles x splits > 0."""
    from mrla_amd import _lib as L
    for b in (1, 2, 8, 256):
        for width in WIDTHS:
            for hw in range(1, 58):
                for s in (1, 2):
                    tn, tc, per, stages, splits, tiles = L.conv3x3_wgrad_plan(b, width, width, hw, hw, s, L.BF16)
                    total = b * ((hw - 1) // s + 1)
                    assert per >= 1 and splits >= 1 and tiles >= 1 and stages >= 1 and tiles * splits > 0
                    assert width % tn == 0 and width % tc == 0 and tiles == (width // tn) * (width // tc)
                    assert (splits - 1) * per < total <= splits * per, (b, width, hw, s, per, splits)      # no gap, no empty split
                    assert tiles * splits <= 1024 or splits == 1


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_of_the_new_file_uses_scratch():
    kernels = kr.kernel_resources("conv3x3_wgrad.hip")
    main = [k for k in kernels if "conv3x3_wgrad_kernel" in k["mangled"]]
    assert len(main) == 4 and any("split_sum_kernel" in k["mangled"] for k in kernels)      # bf16 / fp16 x stride 1 / 2
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"instances with scratch (bytes per lane): {bad}"
    for k in main:           # __launch_bounds__(256, 2): the planner's two workgroups per CU
        assert k["waves"] >= 2, (k["mangled"], k["vgprs"], k["agprs"])


def _conv(cin=64, cout=64, **kw):
    args = dict(kernel_size=3, padding=1, bias=False)
    args.update(kw)
    return torch.nn.Conv2d(cin, cout, **args)


def test_the_switch_is_off_by_default_and_off_means_the_module_itself():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_WGRAD is False
    conv = _conv()
    x = torch.randn(2, 64, 5, 5, requires_grad=True)
    y = Fm.conv3x3(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn).__name__ == type(conv(x).grad_fn).__name__
    with mrla_amd.conv3x3_wgrad():
        assert Fm.CONV3X3_WGRAD is True
        with mrla_amd.conv3x3_wgrad(False):
            assert Fm.CONV3X3_WGRAD is False
        assert Fm.CONV3X3_WGRAD is True
        assert torch.equal(Fm.conv3x3(x, conv), conv(x))          # a CPU tensor: not eligible, the module itself
    assert Fm.CONV3X3_WGRAD is False
    with pytest.raises(RuntimeError):
        with mrla_amd.conv3x3_wgrad():
            raise RuntimeError("x")
    assert Fm.CONV3X3_WGRAD is False                            # the previous value comes back when the block raises


def excluded_configurations():
    """(name, conv, make_x(device)): what conv3x3_applies refuses whatever the device -- shared with the GPU route test."""
    cl = torch.channels_last
    bf = lambda dev: torch.randn(2, 64, 6, 6, device=dev).bfloat16().contiguous(memory_format=cl)  # noqa: E731
    frozen = _conv()
    frozen.weight.requires_grad_(False)
    return [("groups 2", _conv(groups=2), bf), ("dilation 2", _conv(dilation=2, padding=2), bf), ("bias", _conv(bias=True), bf),
            ("stride (2, 1)", _conv(stride=(2, 1)), bf), ("frozen weight", frozen, bf),
            ("fp32", _conv(), lambda dev: torch.randn(2, 64, 6, 6, device=dev).contiguous(memory_format=cl)),
            ("NCHW", _conv(), lambda dev: torch.randn(2, 64, 6, 6, device=dev).bfloat16()),
            ("5x5", _conv(kernel_size=5, padding=2), bf), ("padding 0", _conv(padding=0), bf), ("c = 96", _conv(96, 64), lambda dev: torch.randn(2, 96, 6, 6, device=dev).bfloat16().contiguous(memory_format=cl))]


def test_applies_is_false_for_cpu_tensors_and_every_excluded_configuration():
    from mrla_amd import functional as Fm
    conv = _conv().bfloat16()
    x = torch.randn(2, 64, 6, 6).bfloat16().contiguous(memory_format=torch.channels_last)
    assert not Fm.conv3x3_applies(conv, x)
    for name, c, make in excluded_configurations():
        assert not Fm.conv3x3_applies(c.bfloat16(), make("cpu")), name
