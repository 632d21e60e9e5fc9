"""Host side and compiler side of mrla_stem_conv_f32_wgrad (mrla_amd/csrc/stem_wgrad_f32.hip) and of its switch in the Python
layer.  No GPU: nothing is launched.

  * the three symbols are additive (declared, exported, bound; ABI version 5), and the 16-bit entry points go on refusing
    MRLA_F32;
  * rows, plan and the launch answer the same code for the same arguments: non-positive dimensions, NULL and misaligned
    pointers, n = 96, a shape over the size limit -- which is stated on the real sizes of x and of dy, so train.py's own
    batch 256 at 224 x 224 is served;
  * plan arithmetic: the splits cover b * ho exactly once, the column segments cover wo, the LDS stays within the opt-in limit;
  * the switch: off by default, restored on exit and on raise, set by reproducible_gradients(), left alone by stem_wgrad(),
    conv3x3_wgrad_f32() and conv3x3_wgrad(); stem_conv_f32_applies refuses CPU tensors and every excluded configuration; with
    the switch on, stem_conv of a CPU tensor is the module itself;
  * from the compiler: no kernel of the new file uses scratch."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.test_stem_wgrad_cpu import _conv, excluded_configurations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

SYMBOLS = {"mrla_stem_conv_f32_wgrad_rows": 4, "mrla_stem_conv_f32_wgrad_plan": 5, "mrla_stem_conv_f32_wgrad": 9}
GOOD = (8, 64, 64, 64)
TRAIN = (256, 64, 224, 224)          # resnet/train.py's own batch: dy is 822 MB, x is 154 MB
LDS_OPT_IN = 160 * 1024              # the LDS a workgroup of gfx950 can opt in to
LDS_TWO_PER_CU = 80 * 1024           # kSfLdsCap of stem_wgrad_f32.hip: two workgroups per CU


def test_the_symbols_are_additive():
    from mrla_amd import _lib as L
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    lib = L.load()
    for name, nargs in SYMBOLS.items():
        assert name in L.SIGNATURES and len(L.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name) and re.search(rf"^int {name}\(", header, re.M), name
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and lib.mrla_abi_version() == 5
    assert L.stem_conv_f32_wgrad_plan(*GOOD) is not None
    # the 16-bit entry points keep refusing fp32 operands
    out = (ctypes.c_int * 7)()
    assert lib.mrla_stem_conv_wgrad_rows(*GOOD, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_stem_conv_wgrad_plan(*GOOD, L.F32, ctypes.cast(out, ctypes.c_void_p)) == L.EUNSUPPORTED
    assert lib.mrla_stem_conv_wgrad(16, 32, 48, 64, *GOOD, L.F32, L.F32, None) == L.EUNSUPPORTED


def _all_three(lib, shape):
    """The code rows, plan and launch answer for `shape` (they must agree; rows > 0 and MRLA_OK count as 0).  The launch is only
    asked where the answer is a refusal: nothing is launched."""
    out = (ctypes.c_int * 7)()
    r = lib.mrla_stem_conv_f32_wgrad_rows(*shape)
    p = lib.mrla_stem_conv_f32_wgrad_plan(*shape, ctypes.cast(out, ctypes.c_void_p))
    assert (r if r < 0 else 0) == p, (shape, r, p)
    if r > 0:
        assert out[2] == r
    else:
        assert lib.mrla_stem_conv_f32_wgrad(16, 32, 48, 64, *shape, None) == r, shape
    return p


def test_the_argument_matrix():
    from mrla_amd import _lib as L
    lib = L.load()
    assert _all_three(lib, GOOD) == L.OK and _all_three(lib, TRAIN) == L.OK
    cases = [((8, 96, 64, 64), L.EUNSUPPORTED), ((8, 32, 64, 64), L.EUNSUPPORTED),      # n % 64
             ((512, 64, 256, 256), L.EUNSUPPORTED),         # dy: 512 * 128 * 128 * 64 * 4 = 2^31 bytes (x is 402 MB; with
             #                                                n >= 64, dy is never the smaller of the two)
             ((128, 256, 256, 256), L.EUNSUPPORTED),        # ... through n
             ((0, 64, 64, 64), L.EINVAL), ((-1, 64, 64, 64), L.EINVAL), ((8, 0, 64, 64), L.EINVAL), ((8, -64, 64, 64), L.EINVAL),
             ((8, 64, 0, 64), L.EINVAL), ((8, 64, 64, -1), L.EINVAL)]
    for shape, code in cases:
        assert _all_three(lib, shape) == code, shape
    # just inside the limit on dy (2^31 - 2^22 bytes), and where max(3, n) of the whole of x would have refused
    assert _all_three(lib, (511, 64, 256, 256)) == L.OK and _all_three(lib, (127, 256, 256, 256)) == L.OK
    # any b, h, w >= 1 within that: odd sizes, maps smaller than the kernel, rows wider than one step
    for shape in [(1, 64, 1, 1), (2, 128, 1, 1), (8, 64, 5, 7), (1, 64, 3, 257), (1, 192, 1, 4001), (2, 64, 800, 1344)]:
        assert _all_three(lib, shape) == L.OK, shape
    assert lib.mrla_stem_conv_f32_wgrad_plan(*GOOD, None) == L.EINVAL                              # NULL out


def test_the_launch_refuses_null_and_misaligned_pointers_before_launching():
    from mrla_amd import _lib as L
    lib = L.load()
    ptrs = dict(dy=16, x=32, part=48, dw=64)
    for name in ptrs:
        for bad in (None, ptrs[name] + 4, ptrs[name] + 8):
            a = dict(ptrs)
            a[name] = bad
            assert lib.mrla_stem_conv_f32_wgrad(a["dy"], a["x"], a["part"], a["dw"], *GOOD, None) == L.EINVAL, (name, bad)
    # a bad pointer is invalid also where the shape is unsupported
    assert lib.mrla_stem_conv_f32_wgrad(None, 32, 48, 64, 8, 96, 64, 64, None) == L.EINVAL


def test_rows_equal_the_plans_splits():
    from mrla_amd import _lib as L
    lib = L.load()
    for b, n, h, w in ((1, 64, 1, 1), (1, 64, 5, 7), (2, 64, 9, 6), (3, 128, 14, 10), (5, 64, 40, 40), TRAIN,
                       (64, 64, 224, 224), (16, 64, 224, 224), (2, 64, 800, 1344), (1, 64, 3, 257), (1, 192, 1, 4001)):
        plan = L.stem_conv_f32_wgrad_plan(b, n, h, w)
        assert plan is not None and plan[2] == lib.mrla_stem_conv_f32_wgrad_rows(b, n, h, w) > 0, (b, n, h, w)
        assert plan[0] == 64 and plan[3] == -(-((w - 1) // 2 + 1) // plan[5])


def test_the_splits_tile_the_output_rows_exactly_once_and_the_lds_stays_under_the_cap():
    """b in {1, 2, 8, 256}, n = 64, maps 1 .. 230.  Split i takes the output rows [i * per, min(total, (i + 1) * per)):
    together every row once, none empty."""
    from mrla_amd import _lib as L
    worst = 0
    for b in (1, 2, 8, 256):
        for hw in range(1, 231):
            tn, per, splits, nseg, lds, ws, rmax = L.stem_conv_f32_wgrad_plan(b, 64, hw, hw)
            ho = wo = (hw - 1) // 2 + 1
            total = b * ho
            assert tn == 64 and per >= 1 and splits >= 1 and nseg >= 1 and 1 <= rmax <= ho and 1 <= ws <= wo
            assert (splits - 1) * per < total <= splits * per, (b, hw, per, splits)      # no gap, no empty split
            assert (nseg - 1) * ws < wo <= nseg * ws
            assert 0 < lds <= LDS_TWO_PER_CU <= LDS_OPT_IN, (b, hw, lds)
            worst = max(worst, lds)
    for w in (255, 256, 257, 511, 1344, 4001):                                  # ... and rows cut into column segments
        tn, per, splits, nseg, lds, ws, rmax = L.stem_conv_f32_wgrad_plan(1, 64, 3, w)
        assert nseg >= 1 and (nseg - 1) * ws < (w - 1) // 2 + 1 <= nseg * ws and (nseg == 1 or rmax == 1)
        assert 0 < lds <= LDS_TWO_PER_CU, (w, lds)
        worst = max(worst, lds)
    assert worst > LDS_TWO_PER_CU // 2          # (the cap is the kernel's, not a number far above what it uses)


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_kernel_of_the_new_file_uses_scratch():
    kernels = kr.kernel_resources("stem_wgrad_f32.hip")
    main = [k for k in kernels if "stem_wgrad_f32_kernel" in k["mangled"]]
    assert len(main) == 1 and any("split_sum_kernel" in k["mangled"] for k in kernels)
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"kernels with scratch (bytes per lane): {bad}"
    for k in main:           # __launch_bounds__(256, 2): the planner's two workgroups per CU
        assert k["waves"] >= 2 and k["vgprs"] + k["agprs"] <= 256, (k["mangled"], k["vgprs"], k["agprs"], k["waves"])


def test_the_switch():
    import mrla_amd
    from mrla_amd import functional as Fm
    others = lambda: (Fm.STEM_WGRAD, Fm.CONV3X3_WGRAD, Fm.CONV3X3_WGRAD_F32)  # noqa: E731
    assert Fm.STEM_WGRAD_F32 is False
    assert mrla_amd.stem_wgrad_f32 is Fm.stem_wgrad_f32
    with mrla_amd.stem_wgrad_f32():
        assert Fm.STEM_WGRAD_F32 is True and others() == (False, False, False)
        with mrla_amd.stem_wgrad_f32(False):
            assert Fm.STEM_WGRAD_F32 is False
        assert Fm.STEM_WGRAD_F32 is True
    assert Fm.STEM_WGRAD_F32 is False
    with pytest.raises(RuntimeError, match="inside"):
        with mrla_amd.stem_wgrad_f32():
            raise RuntimeError("inside")
    assert Fm.STEM_WGRAD_F32 is False                           # the previous value comes back when the block raises
    with mrla_amd.reproducible_gradients():
        assert Fm.STEM_WGRAD_F32 is True and others() == (True, True, True)
        with mrla_amd.reproducible_gradients(False):
            assert Fm.STEM_WGRAD_F32 is False
        assert Fm.STEM_WGRAD_F32 is True
    assert Fm.STEM_WGRAD_F32 is False and others() == (False, False, False)
    with mrla_amd.stem_wgrad_f32():
        with pytest.raises(ValueError):
            with mrla_amd.reproducible_gradients():
                raise ValueError
        assert Fm.STEM_WGRAD_F32 is True and others() == (False, False, False)
    assert Fm.STEM_WGRAD_F32 is False
    for other in (mrla_amd.stem_wgrad, mrla_amd.conv3x3_wgrad_f32, mrla_amd.conv3x3_wgrad):
        with other():
            assert Fm.STEM_WGRAD_F32 is False, other.__name__
        with mrla_amd.stem_wgrad_f32(), other(False):
            assert Fm.STEM_WGRAD_F32 is True, other.__name__
    doc = Fm.reproducible_gradients.__doc__
    assert "fp32" in doc and "7x7" in doc and "mrla_stem_conv_f32_wgrad" in doc and "no fp32 stem kernel" not in doc


def test_applies_is_false_for_cpu_tensors_and_every_excluded_configuration():
    from mrla_amd import functional as Fm
    cl = torch.channels_last
    conv = _conv()
    x = torch.randn(2, 3, 12, 12).contiguous(memory_format=cl)
    assert not Fm.stem_conv_f32_applies(conv, x)                                            # a CPU tensor
    for name, c, make in excluded_configurations():
        assert not Fm.stem_conv_f32_applies(c, make("cpu")), name
        assert not Fm.stem_conv_f32_applies(c, make("cpu").float()), name                  # ... nor with an fp32 input
        assert not Fm.stem_conv_applies(c if name.startswith("fp32") else c.bfloat16(), make("cpu")), name
    assert not Fm.stem_conv_f32_applies(conv, x.bfloat16())                                 # bf16 input
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not Fm.stem_conv_f32_applies(conv, x)                                        # fp32 input under bf16 autocast
    frozen = _conv()
    frozen.weight.requires_grad_(False)
    assert not Fm.stem_conv_f32_applies(frozen, x)
    with torch.no_grad():
        assert not Fm.stem_conv_f32_applies(conv, x)


def test_on_means_the_module_itself_for_a_cpu_tensor():
    import mrla_amd
    from mrla_amd import functional as Fm
    conv = _conv()
    x = torch.randn(2, 3, 10, 10, requires_grad=True)
    want = conv(x)
    y = Fm.stem_conv(x, conv)
    assert torch.equal(y, want) and type(y.grad_fn) is type(want.grad_fn)
    with mrla_amd.stem_wgrad_f32():
        y = Fm.stem_conv(x, conv)                                 # a CPU tensor: not eligible, the module itself
        assert torch.equal(y, want) and type(y.grad_fn) is type(want.grad_fn)
    with mrla_amd.stem_wgrad_f32(), mrla_amd.stem_wgrad():
        y = Fm.stem_conv(x, conv)
        assert torch.equal(y, want) and type(y.grad_fn) is type(want.grad_fn)
