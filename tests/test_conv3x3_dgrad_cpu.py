"""Host side and compiler side of mrla_conv3x3_dgrad_s2 (mrla_amd/csrc/conv3x3_dgrad.hip) and of its switch in the Python
layer.  Needs the built library and, for the resource figures, hipcc -- not a GPU.

  * the two symbols are exported, declared and bound, the ABI version is still 5;
  * argument validation: every MRLA_EINVAL / MRLA_EUNSUPPORTED case of the header's contract, decided before any launch, and
    the query answering the launch's codes;
  * the planner: the workgroups' ranges tile the b * ho cell rows exactly once, none empty, workgroups = ranges * c / 64;
  * no scratch in either compiled instance, at least one wave per SIMD;
  * the switch is off by default, off means conv(x) itself, it nests and comes back when the block raises;
    reproducible_gradients() and conv3x3_fwd() leave it alone; conv3x3_dgrad_applies refuses CPU tensors, stride 1, an input
    that wants no gradient and every excluded configuration."""
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
    for name in ("mrla_conv3x3_dgrad_s2_plan", "mrla_conv3x3_dgrad_s2"):
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert L.SIGNATURES["mrla_conv3x3_dgrad_s2_plan"] == [L._I] * 6 + [L._P]
    assert L.SIGNATURES["mrla_conv3x3_dgrad_s2"] == [L._P] * 3 + [L._I] * 6 + [L._P]
    assert re.search(r"^int mrla_conv3x3_dgrad_s2_plan\(int b, int c, int n, int h, int w, int dtype, int\* out\);", header, re.M)
    assert re.search(r"^int mrla_conv3x3_dgrad_s2\(const void\* dy, const void\* wt, void\* dx, int b, int c, int n, int h, int w, "
                     r"int dtype, void\* stream\);", header, re.M)
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5


SHAPE_CASES = [((8, 96, 512, 14, 14), "EUNSUPPORTED"), ((8, 512, 96, 14, 14), "EUNSUPPORTED"),      # c, n % 64
               ((256, 64, 64, 256, 256), "EUNSUPPORTED"), ((64, 64, 256, 256, 256), "EUNSUPPORTED"),      # b*h*w*max(c,n)*2 = 2^31
               ((0, 512, 512, 14, 14), "EINVAL"), ((8, 0, 512, 14, 14), "EINVAL"), ((8, 512, -64, 14, 14), "EINVAL"),
               ((8, 512, 512, 0, 14), "EINVAL"), ((8, 512, 512, 14, -1), "EINVAL")]
GOOD = (8, 512, 512, 14, 14)


def test_the_query_validates_its_arguments():
    from mrla_amd import _lib as L
    plan = L.load().mrla_conv3x3_dgrad_s2_plan
    out = (ctypes.c_int * 6)()
    po = ctypes.cast(out, ctypes.c_void_p)
    for dt in (L.BF16, L.F16):
        assert plan(*GOOD, dt, po) == L.OK and out[0] == 64 and out[5] == out[4] * (512 // 64)
    for args, code in SHAPE_CASES:
        for dt in (L.BF16, L.F16):
            assert plan(*args, dt, po) == getattr(L, code), (args, dt)
    assert plan(255, 64, 64, 256, 256, L.BF16, po) == L.OK                 # just below the bound
    assert plan(*GOOD, L.F32, po) == L.EUNSUPPORTED
    assert plan(*GOOD, 7, po) == L.EINVAL                                   # a dtype code that is none
    assert plan(*GOOD, L.BF16, None) == L.EINVAL                            # null out
    assert L.conv3x3_dgrad_s2_plan(2, 96, 64, 7, 7) is None and L.conv3x3_dgrad_s2_plan(2, 64, 64, 7, 7) is not None


def test_the_launch_validates_its_arguments_before_launching():
    from mrla_amd import _lib as L
    lib = L.load()
    one, two, three = (ctypes.c_void_p(16 * i) for i in (1, 2, 3))
    odd = ctypes.c_void_p(24)
    out = (ctypes.c_int * 6)()
    po = ctypes.cast(out, ctypes.c_void_p)

    def call(dtype, shape=GOOD, dy=one, wt=two, dx=three):
        return lib.mrla_conv3x3_dgrad_s2(dy, wt, dx, *shape, dtype, None)
    # nothing is launched in any of these
    for name in ("dy", "wt", "dx"):
        assert call(L.BF16, **{name: None}) == L.EINVAL, name
        assert call(L.BF16, **{name: odd}) == L.EINVAL, name
        assert call(L.F16, **{name: odd}) == L.EINVAL, name
        assert call(L.F32, **{name: odd}) == L.EINVAL, name
    assert call(7) == L.EINVAL
    assert call(L.F32) == L.EUNSUPPORTED
    for args, code in SHAPE_CASES:
        for dt in (L.BF16, L.F16):
            assert call(dt, shape=args) == getattr(L, code), (args, dt)
            assert call(dt, shape=args) == lib.mrla_conv3x3_dgrad_s2_plan(*args, dt, po)      # the query answers the launch's code


def test_the_ranges_tile_the_cell_rows_exactly_once():
    """b in {1, 2, 8, 256}, the four ResNet widths, maps 1 .. 57.  Range i takes the cell rows [i * per, min(total, (i + 1) *
    per)) of the b * ho: together every cell row once, none empty; a step holds whole rows or one segment; at most 256
    workgroups; a range is at least a full step (two where n = 64, whose weights are loaded once) unless it is the only one."""
    from mrla_amd import _lib as L
    for b in (1, 2, 8, 256):
        for width in WIDTHS:
            for hw in range(1, 58):
                for dt in (L.BF16, L.F16):
                    tc, per, rstep, nseg, ranges, wgs = L.conv3x3_dgrad_s2_plan(b, width, width, hw, hw, dt)
                    ho = (hw - 1) // 2 + 1
                    total = b * ho
                    assert tc == 64 and per >= 1 and ranges >= 1 and 1 <= rstep <= ho and nseg >= 1 and (nseg == 1 or rstep == 1)
                    assert wgs == ranges * (width // tc)
                    assert (ranges - 1) * per < total <= ranges * per, (b, width, hw, per, ranges)      # no gap, no empty range
                    assert ranges <= -(-256 // (width // tc)), (b, width, hw, ranges)
                    assert ranges == 1 or per >= (2 if width == 64 else 1) * rstep, (b, width, hw, per, rstep)
                    assert rstep * (ho + 1) <= 128 or rstep == 1                 # a step's cells, the pad column included
    # rows wider than a step are cut into segments of at most 63 cell columns
    assert L.conv3x3_dgrad_s2_plan(1, 64, 64, 3, 131)[2:4] == (1, 2) and L.conv3x3_dgrad_s2_plan(1, 64, 64, 2, 250)[2:4] == (1, 2)
    assert L.conv3x3_dgrad_s2_plan(1, 64, 64, 2, 126)[3] == 1 and L.conv3x3_dgrad_s2_plan(1, 64, 64, 2, 127)[3] == 2
    # c != n: the tiles are c's, the once-loaded weights n's
    assert L.conv3x3_dgrad_s2_plan(2, 128, 64, 9, 6)[5] == 2 * L.conv3x3_dgrad_s2_plan(2, 128, 64, 9, 6)[4]


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_of_the_new_file_uses_scratch():
    kernels = kr.kernel_resources("conv3x3_dgrad.hip")
    main = [k for k in kernels if "conv3x3_dgrad_s2_kernel" in k["mangled"]]
    assert len(main) == 2 and len(kernels) == 2                # bf16 / fp16
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"instances with scratch (bytes per lane): {bad}"
    for k in main:
        assert k["waves"] >= 1 and k["vgprs"] + k["agprs"] <= 512, (k["mangled"], k["vgprs"], k["agprs"])


def test_the_switch_is_off_by_default_and_off_means_the_module_itself():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.CONV3X3_DGRAD is False
    conv = _conv(stride=2)
    x = torch.randn(2, 64, 5, 5, requires_grad=True)
    y = Fm.conv3x3(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
    with mrla_amd.conv3x3_dgrad():
        assert Fm.CONV3X3_DGRAD is True
        with mrla_amd.conv3x3_dgrad(False):
            assert Fm.CONV3X3_DGRAD is False
        assert Fm.CONV3X3_DGRAD is True
        y = Fm.conv3x3(x, conv)                                    # a CPU tensor: not eligible, the module itself
        assert torch.equal(y, conv(x)) and type(y.grad_fn) is type(conv(x).grad_fn)
        with mrla_amd.reproducible_gradients(False), mrla_amd.conv3x3_fwd(False):
            assert Fm.CONV3X3_DGRAD is True                        # (the other switches leave this one alone, on ...)
    assert Fm.CONV3X3_DGRAD is False
    with pytest.raises(RuntimeError):
        with mrla_amd.conv3x3_dgrad():
            raise RuntimeError("x")
    assert Fm.CONV3X3_DGRAD is False                             # the previous value comes back when the block raises
    with mrla_amd.reproducible_gradients(), mrla_amd.conv3x3_fwd():      # (... and off)
        assert Fm.CONV3X3_DGRAD is False and Fm.CONV3X3_WGRAD and Fm.STEM_WGRAD and Fm.CONV3X3_FWD
    with mrla_amd.conv3x3_dgrad():                               # ... and it leaves them alone
        assert not (Fm.CONV3X3_WGRAD or Fm.STEM_WGRAD or Fm.CONV3X3_FWD)
    assert mrla_amd.conv3x3_dgrad is Fm.conv3x3_dgrad


def test_applies_is_false_for_cpu_tensors_stride_1_and_every_excluded_configuration():
    from mrla_amd import functional as Fm
    cl = torch.channels_last
    conv = _conv(stride=2).bfloat16()
    x = torch.randn(2, 64, 6, 6).bfloat16().contiguous(memory_format=cl).requires_grad_(True)
    assert not Fm.conv3x3_dgrad_applies(conv, x)                 # a CPU tensor
    for name, c, make in excluded_configurations():
        assert not Fm.conv3x3_dgrad_applies(c.bfloat16(), make("cpu").requires_grad_(True)), name

    # apart from the device check: the same tensors claiming to be CUDA tensors (no GPU here; is_cuda is all the check reads
    # of the device)
    class _OnDevice(torch.Tensor):
        is_cuda = True

    def claim(t):
        return t.as_subclass(_OnDevice)

    def on_device(c):
        c = c.bfloat16()
        c.weight = torch.nn.Parameter(claim(c.weight.data), requires_grad=c.weight.requires_grad)
        return c
    for name, c, make in excluded_configurations():              # (all of them at stride 1 or (2, 1))
        assert not Fm.conv3x3_dgrad_applies(on_device(c), claim(make("cpu")).requires_grad_(True)), name
    good = on_device(_conv(stride=2))
    xd = claim(x.detach()).requires_grad_(True)
    assert Fm.conv3x3_dgrad_applies(good, xd)
    assert not Fm.conv3x3_dgrad_applies(good, claim(x.detach()))             # an input that wants no gradient
    with torch.no_grad():
        assert not Fm.conv3x3_dgrad_applies(good, xd)
    assert not Fm.conv3x3_dgrad_applies(on_device(_conv()), xd)              # stride 1
    assert not Fm.conv3x3_dgrad_applies(on_device(_conv(stride=(2, 1))), xd)
    frozen = on_device(_conv(stride=2))
    frozen.weight.requires_grad_(False)
    assert Fm.conv3x3_dgrad_applies(frozen, xd)                              # a frozen weight still has an input gradient
    for bad in (_conv(stride=2, groups=2), _conv(stride=2, dilation=2, padding=2), _conv(stride=2, bias=True),
                _conv(stride=2, kernel_size=5, padding=2), _conv(stride=2, padding=0)):
        assert not Fm.conv3x3_dgrad_applies(on_device(bad), xd)
    assert not Fm.conv3x3_dgrad_applies(good, claim(x.detach().float()).requires_grad_(True))                   # fp32
    assert not Fm.conv3x3_dgrad_applies(good, claim(x.detach().contiguous()).requires_grad_(True))             # NCHW
    x96 = claim(torch.randn(2, 96, 6, 6).bfloat16().contiguous(memory_format=cl)).requires_grad_(True)
    assert not Fm.conv3x3_dgrad_applies(on_device(_conv(96, 64, stride=2)), x96)                              # c = 96
