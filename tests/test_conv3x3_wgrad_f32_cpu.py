"""Host side and compiler side of mrla_conv3x3_f32_wgrad (mrla_amd/csrc/conv3x3_wgrad_f32.hip) and of its switch in the Python
layer.  Needs the built library and, for the resource figures, hipcc -- not a GPU.

  * the three symbols are exported, declared and bound with 6 / 7 / 11 arguments, additive (the ABI version stays 5);
  * argument validation: every MRLA_EINVAL / MRLA_EUNSUPPORTED case of the header's contract, decided before any launch, rows,
    plan and launch answering the same code;
  * the planner over the GPU test's shapes and ResNet-50's seven 3x3 shapes at batch 64 and 256: splits = ceil(b * ho / rows
    per split) = rows of part, no empty split, tiles = (n / tile n) * (c / tile c);
  * no scratch in any compiled instance, and the two waves per SIMD of __launch_bounds__(256, 2);
  * the switch: off by default, restored on exit and on raise, set by reproducible_gradients(), left alone by conv3x3_wgrad()
    and conv3x3_wgrad_auto(); off means conv(x) itself; conv3x3_f32_applies refuses CPU tensors and every excluded
    configuration."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.test_conv3x3_wgrad_cpu import _conv, excluded_configurations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

SYMBOLS = {"mrla_conv3x3_f32_wgrad_rows": 6, "mrla_conv3x3_f32_wgrad_plan": 7, "mrla_conv3x3_f32_wgrad": 11}
GPU_SHAPES = [(1, 64, 64, 1, 1, 1), (1, 64, 64, 2, 1, 2), (1, 64, 64, 3, 5, 1), (2, 64, 128, 7, 7, 1), (3, 128, 64, 8, 33, 1),
              (2, 64, 64, 7, 7, 2), (2, 64, 64, 9, 6, 2), (1, 128, 128, 14, 14, 2), (2, 256, 256, 14, 14, 1), (5, 64, 64, 28, 28, 1),
              (8, 512, 512, 7, 7, 1), (8, 512, 512, 14, 14, 2), (1, 64, 64, 2, 70, 1), (1, 64, 64, 3, 131, 2)]
RESNET50 = [(64, 56, 1), (128, 56, 2), (128, 28, 1), (256, 28, 2), (256, 14, 1), (512, 14, 2), (512, 7, 1)]     # (width, input side, stride)
GOOD = (8, 512, 512, 7, 7, 1)


def test_the_gpu_shapes_are_the_gpu_tests():
    from tests.test_conv3x3_wgrad_gpu import SHAPES
    assert GPU_SHAPES == SHAPES


def test_the_symbols_are_additive():
    from mrla_amd import _lib as L
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    lib = L.load()
    for name, nargs in SYMBOLS.items():
        assert name in L.SIGNATURES and len(L.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name) and re.search(rf"^int {name}\(", header, re.M), name
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and lib.mrla_abi_version() == 5
    assert L.conv3x3_f32_wgrad_plan(*GOOD) is not None
    # the 16-bit entry points keep refusing fp32 operands
    out = (ctypes.c_int * 6)()
    assert lib.mrla_conv3x3_wgrad_rows(*GOOD, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_conv3x3_wgrad_plan(*GOOD, L.F32, ctypes.cast(out, ctypes.c_void_p)) == L.EUNSUPPORTED
    assert lib.mrla_conv3x3_wgrad(16, 32, 48, 64, *GOOD, L.F32, L.F32, None) == L.EUNSUPPORTED


def _all_three(lib, shape):
    """The code rows, plan and launch answer for `shape` (they must agree; rows > 0 and MRLA_OK count as 0).  The launch is only
    asked where the answer is a refusal: nothing is launched."""
    out = (ctypes.c_int * 6)()
    r = lib.mrla_conv3x3_f32_wgrad_rows(*shape)
    p = lib.mrla_conv3x3_f32_wgrad_plan(*shape, ctypes.cast(out, ctypes.c_void_p))
    assert (r if r < 0 else 0) == p, (shape, r, p)
    if r > 0:
        assert out[4] == r
    else:
        assert lib.mrla_conv3x3_f32_wgrad(16, 32, 48, 64, *shape, None) == r, shape
    return p


def test_the_argument_matrix():
    from mrla_amd import _lib as L
    lib = L.load()
    assert _all_three(lib, GOOD) == L.OK
    cases = [((8, 96, 512, 7, 7, 1), L.EUNSUPPORTED), ((8, 512, 32, 7, 7, 1), L.EUNSUPPORTED),      # c = 96, n = 32
             ((8, 512, 96, 7, 7, 1), L.EUNSUPPORTED), ((8, 32, 512, 7, 7, 2), L.EUNSUPPORTED),
             ((8, 512, 512, 7, 7, 3), L.EUNSUPPORTED), ((8, 512, 512, 7, 7, 4), L.EUNSUPPORTED),    # other strides
             ((128, 64, 64, 256, 256, 1), L.EUNSUPPORTED),             # b*h*w*max(c, n)*4 = 2^31 through c
             ((32, 64, 256, 256, 256, 2), L.EUNSUPPORTED),             # ... through n
             ((0, 512, 512, 7, 7, 1), L.EINVAL), ((-1, 512, 512, 7, 7, 1), L.EINVAL), ((8, 0, 512, 7, 7, 1), L.EINVAL),
             ((8, 512, -64, 7, 7, 1), L.EINVAL), ((8, 512, 512, 0, 7, 1), L.EINVAL), ((8, 512, 512, 7, -1, 1), L.EINVAL),
             ((8, 512, 512, 7, 7, 0), L.EINVAL), ((8, 512, 512, 7, 7, -2), L.EINVAL)]
    for shape, code in cases:
        assert _all_three(lib, shape) == code, shape
    # just inside the limit: 2^31 - 2^24 bytes, through c and through n
    assert _all_three(lib, (127, 64, 64, 256, 256, 1)) == L.OK and _all_three(lib, (31, 64, 256, 256, 256, 2)) == L.OK
    # any b, h, w >= 1 within that: odd sizes, maps smaller than the kernel, rows wider than one step
    for shape in [(1, 64, 64, 1, 1, 1), (1, 64, 64, 1, 1, 2), (3, 64, 64, 2, 1, 2), (1, 64, 64, 1, 4000, 2), (1, 64, 64, 3, 1001, 1)]:
        assert _all_three(lib, shape) == L.OK, shape
    assert lib.mrla_conv3x3_f32_wgrad_plan(*GOOD, None) == L.EINVAL                              # NULL out


def test_the_launch_refuses_null_and_misaligned_pointers_before_launching():
    from mrla_amd import _lib as L
    lib = L.load()
    ptrs = dict(dy=16, x=32, part=48, dw=64)
    for name in ptrs:
        for bad in (None, ptrs[name] + 4, ptrs[name] + 8):
            a = dict(ptrs)
            a[name] = bad
            assert lib.mrla_conv3x3_f32_wgrad(a["dy"], a["x"], a["part"], a["dw"], *GOOD, None) == L.EINVAL, (name, bad)
    # a bad pointer is invalid also where the shape is unsupported
    assert lib.mrla_conv3x3_f32_wgrad(None, 32, 48, 64, 8, 96, 512, 7, 7, 1, None) == L.EINVAL


def _plan_shapes():
    return GPU_SHAPES + [(b, wd, wd, side, side, s) for b in (64, 256) for wd, side, s in RESNET50]


def test_plan_invariants():
    from mrla_amd import _lib as L
    lib = L.load()
    for shape in _plan_shapes():
        b, c, n, h, w, s = shape
        plan = L.conv3x3_f32_wgrad_plan(*shape)
        assert plan is not None, shape
        tn, tc, per, stages, splits, tiles = plan
        total = b * ((h - 1) // s + 1)
        assert per >= 1 and stages >= 1 and n % tn == 0 and c % tc == 0
        assert splits == -(-total // per), shape
        assert (splits - 1) * per < total, shape                       # no empty split
        assert tiles == (n // tn) * (c // tc), shape
        assert lib.mrla_conv3x3_f32_wgrad_rows(*shape) == splits, shape


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_uses_scratch_and_each_reaches_its_launch_bounds():
    kernels = kr.kernel_resources("conv3x3_wgrad_f32.hip")
    main = [k for k in kernels if "conv3x3_wgrad_f32_kernel" in k["mangled"]]
    assert len(main) == 2 and any("split_sum_kernel" in k["mangled"] for k in kernels)      # stride 1 / 2
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"instances with scratch (bytes per lane): {bad}"
    for k in main:           # __launch_bounds__(256, 2): two workgroups of four waves per CU
        assert k["waves"] >= 2 and k["vgprs"] + k["agprs"] <= 256, (k["mangled"], k["vgprs"], k["agprs"], k["waves"])


def test_the_switch():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_WGRAD_F32 is False
    assert mrla_amd.conv3x3_wgrad_f32 is Fm.conv3x3_wgrad_f32
    with mrla_amd.conv3x3_wgrad_f32():
        assert Fm.CONV3X3_WGRAD_F32 is True and Fm.CONV3X3_WGRAD is False and Fm.STEM_WGRAD is False
        with mrla_amd.conv3x3_wgrad_f32(False):
            assert Fm.CONV3X3_WGRAD_F32 is False
        assert Fm.CONV3X3_WGRAD_F32 is True
    assert Fm.CONV3X3_WGRAD_F32 is False
    with pytest.raises(RuntimeError, match="inside"):
        with mrla_amd.conv3x3_wgrad_f32():
            raise RuntimeError("inside")
    assert Fm.CONV3X3_WGRAD_F32 is False                        # the previous value comes back when the block raises
    with mrla_amd.reproducible_gradients():
        assert Fm.CONV3X3_WGRAD_F32 is True and Fm.CONV3X3_WGRAD is True and Fm.STEM_WGRAD is True
        with mrla_amd.reproducible_gradients(False):
            assert Fm.CONV3X3_WGRAD_F32 is False
        assert Fm.CONV3X3_WGRAD_F32 is True
    assert Fm.CONV3X3_WGRAD_F32 is False and Fm.CONV3X3_WGRAD is False and Fm.STEM_WGRAD is False
    with pytest.raises(ValueError):
        with mrla_amd.reproducible_gradients():
            raise ValueError
    assert Fm.CONV3X3_WGRAD_F32 is False
    with mrla_amd.conv3x3_wgrad():
        assert Fm.CONV3X3_WGRAD_F32 is False
    with mrla_amd.conv3x3_wgrad_auto():
        assert Fm.CONV3X3_WGRAD_F32 is False
    with mrla_amd.conv3x3_wgrad_auto(False):
        assert Fm.CONV3X3_WGRAD_F32 is False
    assert "fp32" in Fm.reproducible_gradients.__doc__ and "7x7" in Fm.reproducible_gradients.__doc__


def test_applies_is_false_for_cpu_tensors_and_every_excluded_configuration():
    from mrla_amd import functional as Fm
    cl = torch.channels_last
    conv = _conv()
    x = torch.randn(2, 64, 6, 6).contiguous(memory_format=cl)
    assert not Fm.conv3x3_f32_applies(conv, x)                                              # a CPU tensor
    for name, c, make in excluded_configurations():
        if name == "fp32":
            continue
        assert not Fm.conv3x3_f32_applies(c, make("cpu")), name
        assert not Fm.conv3x3_f32_applies(c, make("cpu").float()), name                    # ... nor with an fp32 input
    assert not Fm.conv3x3_f32_applies(conv, x.bfloat16())                                   # bf16 input
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not Fm.conv3x3_f32_applies(conv, x)                                          # fp32 input under bf16 autocast
    frozen = _conv()
    frozen.weight.requires_grad_(False)
    assert not Fm.conv3x3_f32_applies(frozen, x)
    with torch.no_grad():
        assert not Fm.conv3x3_f32_applies(conv, x)


def test_off_means_the_module_itself():
    import mrla_amd
    from mrla_amd import functional as Fm
    conv = _conv()
    x = torch.randn(2, 64, 5, 5, requires_grad=True).contiguous(memory_format=torch.channels_last)
    y = Fm.conv3x3(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
    with mrla_amd.conv3x3_wgrad_f32():
        y = Fm.conv3x3(x, conv)                                   # a CPU tensor: not eligible, the module itself
        assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
