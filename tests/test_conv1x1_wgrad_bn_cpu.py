"""Host side and compiler side of mrla_conv1x1_wgrad_bn (the BatchNorm backward apply inside the weight-gradient GEMM,
mrla_amd/csrc/conv1x1_wgrad.hip).  Needs the built library and hipcc, not a GPU.

The resource bounds are conditions of the design, not measurements:
  * scratch = 0: the kernel streams over pixel chunks, a spill would be scratch traffic inside that loop;
  * >= 1 wave per SIMD: the launch is one four-wave workgroup per CU (its LDS stages, not a second workgroup, hide the
    latency), and the fused form's largest stage set is the whole LDS of a CU;
  * the plain instances keep the register file they had (the counts of the parent commit): the fused form is a template
    flag on the same body and must not cost the plain form anything."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

TILES = [(64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (128, 256), (256, 64), (256, 128)]
# (VGPRs, AGPRs) of conv1x1_wgrad_kernel<TN, TK, 4, 32> before the fused form existed, bf16 and fp16 alike
PLAIN = {(64, 64): (25, 16), (64, 128): (36, 32), (64, 256): (47, 64), (128, 64): (36, 32), (128, 128): (45, 64),
         (128, 256): (66, 128), (256, 64): (47, 64), (256, 128): (66, 128)}


def test_symbols_and_queries():
    from mrla_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "mrla_conv1x1_wgrad_bn") and hasattr(lib, "mrla_conv1x1_wgrad_bn_supported")
    b = 256
    # resnet50 at batch 256: (m, k, n) of conv3, conv1 and the downsample convolutions of the four stages, and whether the
    # fused form is the faster route there (profiles/wgrad_bn.md section 6: one k-tile, or two with n <= 512)
    classes = []
    for hw, planes, inpl in ((56, 64, 64), (28, 128, 256), (14, 256, 512), (7, 512, 1024)):
        m = b * hw * hw
        classes += [(m, planes, 4 * planes), (m, 4 * planes, planes), (m, inpl, 4 * planes)]
    classes += [(b * 56 * 56, 256, 128), (b * 28 * 28, 512, 256), (b * 14 * 14, 1024, 512)]   # conv1 of a strided first block
    classes.append((b * 56 * 56, 64, 64))                # conv1 of the first block of all
    taken = {(m, k, n) for m, k, n in classes if k <= 256 or (k == 512 and n <= 512)}
    assert len(taken) == 9 and (b * 14 * 14, 256, 1024) in taken and (b * 7 * 7, 512, 2048) not in taken
    for m, k, n in classes:
        for dt in (L.BF16, L.F16):
            assert lib.mrla_conv1x1_wgrad_rows(m, k, n, dt) > 0
            want = 1 if (m, k, n) in taken else L.EUNSUPPORTED
            assert lib.mrla_conv1x1_wgrad_bn_supported(m, k, n, dt) == want, (m, k, n, dt)
    # the rule itself, from the plan: k-tiles = k / tile k
    for k, n in ((256, 2048), (512, 512), (512, 1024), (768, 64), (1024, 64), (384, 256)):
        plan = L.conv1x1_wgrad_plan(4096, k, n, L.BF16)
        ktiles = k // plan[3]
        want = 1 if ktiles == 1 or (ktiles == 2 and n <= 512) else L.EUNSUPPORTED
        assert lib.mrla_conv1x1_wgrad_bn_supported(4096, k, n, L.BF16) == want, (k, n, ktiles)
    one = ctypes.c_void_p(16)              # the launch refuses what the query refuses
    assert lib.mrla_conv1x1_wgrad_bn(one, one, one, one, one, 1, ctypes.c_void_p(32), one, one, one, 4096, 1024, 64, L.BF16,
                                     L.F32, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad_bn_supported(64, 96, 64, L.BF16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad_bn_supported(1 << 24, 128, 64, L.BF16) == L.EUNSUPPORTED       # 32-bit buffer offsets
    assert lib.mrla_conv1x1_wgrad_bn_supported(1000, 64, 64, L.F32) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad_bn_supported(0, 64, 64, L.BF16) == L.EINVAL


def test_argument_validation():
    from mrla_amd import _lib as L
    lib = L.load()
    one = ctypes.c_void_p(16)

    def call(dtype, dw_dtype, g=one, dy_out=ctypes.c_void_p(32), m=64, xb=one, sc=one, sh=one, cb=one):
        return lib.mrla_conv1x1_wgrad_bn(g, xb, sc, sh, cb, 1, dy_out, one, one, one, m, 64, 64, dtype, dw_dtype, None)
    # nothing is launched in any of these
    assert call(L.BF16, L.F16) == L.EINVAL and call(L.F16, L.BF16) == L.EINVAL          # mixed 16-bit dw_dtype
    assert call(L.F32, L.F32) == L.EUNSUPPORTED
    assert call(L.BF16, L.BF16, g=None) == L.EINVAL and call(L.BF16, L.BF16, dy_out=None) == L.EINVAL
    assert call(L.BF16, L.F32, m=0) == L.EINVAL
    # the lanes read sc, sh and cb as float4; dy_out is written while g and xb are still being read
    odd = ctypes.c_void_p(24)
    assert call(L.BF16, L.F32, sc=odd) == L.EINVAL and call(L.BF16, L.F32, sh=odd) == L.EINVAL
    assert call(L.F16, L.F32, cb=odd) == L.EINVAL
    assert call(L.BF16, L.F32, dy_out=one) == L.EINVAL and call(L.BF16, L.F32, dy_out=odd, xb=odd) == L.EINVAL
    # the sequence entry accepts dx == NULL, and still refuses what it refused
    assert lib.mrla_bn_bwd(one, one, one, None, one, 1, 0, L.BN_TRAIN, 0, one, None, 2, 64, 4, 4, L.BF16, L.NHWC, None) == L.EINVAL


pytestmark_hipcc = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")


@pytest.fixture(scope="module")
def instances():
    out = {}
    for k in kr.kernel_resources("conv1x1_wgrad.hip"):
        m = re.search(r"conv1x1_wgrad(_bn)?(_f16)?_kernelILi(\d+)ELi(\d+)ELi4ELi32EEE", k["mangled"])
        if m:
            out[(m.group(1) is not None, m.group(2) is not None, int(m.group(3)), int(m.group(4)))] = k
    return out


@pytestmark_hipcc
def test_every_launched_instance_is_compiled(instances):
    want = {(bn, f16, tn, tk) for bn in (False, True) for f16 in (False, True) for tn, tk in TILES}
    assert want <= set(instances), sorted(want - set(instances))


@pytestmark_hipcc
def test_no_instance_spills_and_one_workgroup_per_cu_fits(instances):
    for key, k in sorted(instances.items()):
        assert k["scratch"] == 0, f"{key}: {k['scratch']} bytes of scratch per lane"
        assert k["waves"] >= 1, f"{key}: {k['vgprs']} VGPRs + {k['agprs']} AGPRs do not fit one wave per SIMD"
        assert k["vgprs"] + k["agprs"] <= 512, key


@pytestmark_hipcc
def test_plain_instances_keep_their_registers(instances):
    for (bn, f16, tn, tk), k in sorted(instances.items()):
        if not bn:
            assert (k["vgprs"], k["agprs"]) == PLAIN[(tn, tk)], ((f16, tn, tk), k["vgprs"], k["agprs"])
