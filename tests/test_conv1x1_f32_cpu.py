"""Host-side gates on the fp32 1x1-convolution GEMMs (mrla_conv1x1_f32_*; mrla_amd/csrc/conv1x1_f32.hip).  No GPU needed:
the queries and the argument checks answer on the host before anything is launched.

  * the five symbols are exported, declared and bound, and additive: the ABI version stays 5 and the existing
    mrla_conv1x1_* entry points go on answering MRLA_EUNSUPPORTED for MRLA_F32;
  * the supported set: every 1x1 convolution of ResNet-50 at batch 256 and at the detection shape 2 x 3 x 800 x 1344, in
    all three products; k or n off the 64 grid, k > 2048 and offsets past 2^31 bytes are refused;
  * MRLA_EINVAL for NULL pointers, pointers that are 4- but not 16-byte aligned, and m = 0;
  * no kernel instance spills (the compiler's resource report; needs hipcc);
  * the Python switch: off by default, conv1x1_applies refuses fp32 while it is off, fp32_gemms() restores the previous
    value on exit and on an exception."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

SYMBOLS = {"mrla_conv1x1_f32_rows": 3, "mrla_conv1x1_f32_plan": 4, "mrla_conv1x1_f32_fwd": 9,
           "mrla_conv1x1_f32_wgrad_rows": 3, "mrla_conv1x1_f32_wgrad": 8}


def resnet50_1x1_shapes(batch, height, width):
    """(m, k, n) of every 1x1 convolution of ResNet-50 (bottlenecks [3, 4, 6, 3], stride on conv2) for a batch of images."""
    h, w = (height + 3) // 4, (width + 3) // 4                  # behind the stem and its pooling
    shapes, inplanes = set(), 64
    for stage, planes in enumerate((64, 128, 256, 512)):
        hi, wi = h, w                                           # the stage's input
        if stage:
            h, w = (h + 1) // 2, (w + 1) // 2
        shapes.add((batch * hi * wi, inplanes, planes))         # conv1 of the first block (conv2 carries the stride)
        shapes.add((batch * h * w, inplanes, 4 * planes))       # its downsample, on the subsampled input
        shapes.add((batch * h * w, planes, 4 * planes))         # conv3
        shapes.add((batch * h * w, 4 * planes, planes))         # conv1 of the other blocks
        inplanes = 4 * planes
    return sorted(shapes)


def test_the_symbols_are_additive():
    from mrla_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mrla_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        assert name in L.SIGNATURES and len(L.SIGNATURES[name]) == nargs, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5
    lib = L.load()
    assert lib.mrla_abi_version() == 5
    for name in SYMBOLS:
        assert hasattr(lib, name)
    # the existing entry points keep refusing fp32 operands
    p = 16
    assert lib.mrla_conv1x1_rows(64, 64, 64, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_fwd(p, p, p, None, 64, 64, 64, L.F32, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad_rows(64, 64, 64, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 64, 64, L.F32, L.F32, None) == L.EUNSUPPORTED


@pytest.mark.parametrize("images", [(256, 224, 224), (2, 800, 1344)], ids=lambda s: "x".join(map(str, s)))
def test_every_resnet50_1x1_is_taken(images):
    from mrla_amd import _lib as L
    lib = L.load()
    shapes = resnet50_1x1_shapes(*images)
    assert len(shapes) >= 13 and max(m * max(k, n) for m, k, n in shapes) * 4 < 2 ** 31
    if images[0] == 256:
        assert (802816, 64, 256) in shapes and (12544, 2048, 512) in shapes and (50176, 512, 1024) in shapes
    for m, k, n in shapes:
        assert lib.mrla_conv1x1_f32_rows(m, k, n) > 0, (m, k, n)             # forward
        assert lib.mrla_conv1x1_f32_rows(m, n, k) > 0, (m, k, n)             # input gradient: the roles of k and n swapped
        assert lib.mrla_conv1x1_f32_wgrad_rows(m, k, n) > 0, (m, k, n)
        plan = L.conv1x1_f32_plan(m, k, n)
        assert plan is not None and plan[0] in (0, 1, 2, 4, 5) and plan[3] == lib.mrla_conv1x1_f32_rows(m, k, n)
        assert (plan[0] >= 4) == (k > 256)


def test_shapes_off_the_supported_set_are_refused():
    from mrla_amd import _lib as L
    lib = L.load()
    for m, k, n in [(64, 96, 64), (64, 64, 96), (64, 4096, 64), (64, 32, 64), (1 << 24, 128, 64), (1 << 24, 64, 128)]:
        assert lib.mrla_conv1x1_f32_rows(m, k, n) == L.EUNSUPPORTED, (m, k, n)
        assert lib.mrla_conv1x1_f32_wgrad_rows(m, k, n) == L.EUNSUPPORTED, (m, k, n)
        assert L.conv1x1_f32_plan(m, k, n) is None
        assert lib.mrla_conv1x1_f32_fwd(16, 16, 0, 16, None, m, k, n, None) == L.EUNSUPPORTED
        assert lib.mrla_conv1x1_f32_wgrad(16, 16, 16, 16, m, k, n, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_f32_rows((1 << 22) - 1, 128, 64) > 0            # just inside the offset limit
    assert lib.mrla_conv1x1_f32_rows(1, 2048, 64) == 1 and lib.mrla_conv1x1_f32_rows(1, 64, 4096) == 1
    # more weight slices than a grid dimension takes: refused on the host, not by the launch
    assert lib.mrla_conv1x1_f32_rows(1, 256, 64 * 65535) == 1 and lib.mrla_conv1x1_f32_rows(1, 256, 64 * 65536) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_f32_fwd(16, 16, 0, 16, None, 1, 256, 64 * 65536, None) == L.EUNSUPPORTED


def test_bad_arguments_are_invalid_before_any_launch():
    from mrla_amd import _lib as L
    lib = L.load()
    ok, off4 = 4096, 4096 + 4
    for m, k, n in [(0, 64, 64), (64, 0, 64), (64, 64, -64)]:
        assert lib.mrla_conv1x1_f32_rows(m, k, n) == L.EINVAL
        assert lib.mrla_conv1x1_f32_wgrad_rows(m, k, n) == L.EINVAL
        assert lib.mrla_conv1x1_f32_fwd(ok, ok, 0, ok, None, m, k, n, None) == L.EINVAL
        assert lib.mrla_conv1x1_f32_wgrad(ok, ok, ok, ok, m, k, n, None) == L.EINVAL
    assert lib.mrla_conv1x1_f32_plan(64, 64, 64, None) == L.EINVAL
    for bad in (None, off4):
        for pos in range(3):                                    # x, w, y
            a = [ok, ok, ok]
            a[pos] = bad
            assert lib.mrla_conv1x1_f32_fwd(a[0], a[1], 0, a[2], None, 64, 64, 64, None) == L.EINVAL, (bad, pos)
        for pos in range(4):                                    # dy, x, part, dw
            a = [ok, ok, ok, ok]
            a[pos] = bad
            assert lib.mrla_conv1x1_f32_wgrad(*a, 64, 64, 64, None) == L.EINVAL, (bad, pos)
    assert lib.mrla_conv1x1_f32_fwd(ok, ok, 0, ok, off4, 64, 64, 64, None) == L.EINVAL        # mom_part: NULL or aligned
    assert lib.mrla_conv1x1_f32_fwd(ok, ok, 2, ok, None, 64, 64, 64, None) == L.EINVAL        # w_trans is 0 or 1


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_spills():
    fwd, wgrad = {}, []
    for k in kr.kernel_resources("conv1x1_f32.hip"):
        m = re.search(r"conv1x1_f32_fwd_kernelILi(\d+)ELb([01])ELb([01])E", k["mangled"])      # <WN, MOM, STREAM>
        if m:
            fwd[tuple(int(v) for v in m.groups())] = k
        elif "conv1x1_f32_wgrad_kernel" in k["mangled"]:
            wgrad.append(k)
    # launch_conv1x1_f32_fwd: resident weights with 1, 2, 4 channel groups, streamed with 1, 2; each with and without records
    assert set(fwd) == {(wn, mo, 0) for wn in (1, 2, 4) for mo in (0, 1)} | {(wn, mo, 1) for wn in (1, 2) for mo in (0, 1)}
    assert len(wgrad) == 1
    for k in list(fwd.values()) + wgrad:
        assert k["scratch"] == 0, (k["mangled"], k["scratch"])
        assert k["vgprs"] + k["agprs"] <= 512 and k["waves"] >= 1


class _Description:
    """What conv1x1_applies asks of its input, for a channels_last CUDA tensor that no machine without a GPU can make."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

    def dim(self):
        return len(self.shape)

    def is_contiguous(self, memory_format=torch.contiguous_format):
        return memory_format == torch.channels_last

    def data_ptr(self):
        return 4096


def test_the_switch_is_off_by_default_and_gates_the_dispatch():
    from mrla_amd import functional as Fm
    assert Fm.CONV1X1_F32 is False
    conv = torch.nn.Conv2d(256, 64, 1, bias=False)
    down = torch.nn.Conv2d(256, 512, 1, stride=2, bias=False)
    x = _Description((2, 256, 14, 14), torch.float32)
    assert not Fm.conv1x1_applies(conv, x) and not Fm.conv1x1_applies(down, x, True)
    assert not Fm.conv1x1_applies(conv, torch.zeros(2, 256, 14, 14).contiguous(memory_format=torch.channels_last))
    with Fm.fp32_gemms():
        assert Fm.CONV1X1_F32 is True
        assert Fm.conv1x1_applies(conv, x) and Fm.conv1x1_applies(down, x, True)
        assert not Fm.conv1x1_applies(torch.nn.Conv2d(96, 64, 1, bias=False), _Description((2, 96, 14, 14), torch.float32))
        assert not Fm.conv1x1_applies(torch.nn.Conv2d(256, 64, 1, bias=False).double(), x)                     # the weight is not fp32
        assert not Fm.conv1x1_applies(conv, torch.zeros(2, 256, 14, 14).contiguous(memory_format=torch.channels_last))
        with Fm.fp32_gemms(False):
            assert Fm.CONV1X1_F32 is False
        assert Fm.CONV1X1_F32 is True
    assert Fm.CONV1X1_F32 is False


def test_fp32_gemms_restores_the_switch_on_an_exception():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert mrla_amd.fp32_gemms is Fm.fp32_gemms
    with pytest.raises(RuntimeError, match="inside"):
        with Fm.fp32_gemms():
            assert Fm.CONV1X1_F32 is True
            raise RuntimeError("inside")
    assert Fm.CONV1X1_F32 is False
    Fm.CONV1X1_F32 = True
    try:
        with pytest.raises(ValueError):
            with Fm.fp32_gemms(False):
                assert Fm.CONV1X1_F32 is False
                raise ValueError
        assert Fm.CONV1X1_F32 is True
    finally:
        Fm.CONV1X1_F32 = False
