"""Host side and compiler side of mrla_conv1x1_wgrad_bn_dx (the BatchNorm backward apply AND the input-gradient GEMM inside
the weight-gradient GEMM, mrla_amd/csrc/conv1x1_wgrad.hip).  Needs the built library and hipcc, not a GPU.

The resource bounds are conditions of the design, not measurements:
  * scratch = 0 and >= 1 wave per SIMD for the new instances (one four-wave workgroup per CU: the 512-entry register file of a
    lane is theirs, and they use it -- 64 registers of W^T fragments stay live across the chunk loop);
  * every plain and every BN instance keeps the registers the parent commit's compiler run gave it: the dX form is a template
    flag on the same body and must not cost the other two forms anything."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

TILES = [(64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (128, 256), (256, 64), (256, 128)]
# (VGPRs, AGPRs, waves per SIMD) on the parent commit, scratch 0 everywhere.  Plain: bf16 and fp16 alike.
PLAIN = {(64, 64): (25, 16, 8), (64, 128): (36, 32, 7), (64, 256): (47, 64, 4), (128, 64): (36, 32, 7),
         (128, 128): (45, 64, 4), (128, 256): (66, 128, 2), (256, 64): (47, 64, 4), (256, 128): (66, 128, 2)}
BN_BF16 = {(64, 64): (69, 16, 5), (64, 128): (79, 32, 4), (64, 256): (90, 64, 3), (128, 64): (86, 32, 4),
           (128, 128): (91, 64, 3), (128, 256): (110, 128, 2), (256, 64): (113, 64, 2), (256, 128): (125, 128, 2)}
BN_F16 = {(64, 64): (68, 16, 5), (64, 128): (79, 32, 4), (64, 256): (90, 64, 3), (128, 64): (85, 32, 4),
          (128, 128): (90, 64, 3), (128, 256): (110, 128, 2), (256, 64): (112, 64, 2), (256, 128): (124, 128, 2)}


def test_symbols_are_exported_and_declared():
    from mrla_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "mrla_conv1x1_wgrad_bn_dx") and hasattr(lib, "mrla_conv1x1_wgrad_bn_dx_supported")
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint mrla_conv1x1_wgrad_bn_dx_supported\(int m, int k, int n, int dtype\);", header)
    assert re.search(r"\bint mrla_conv1x1_wgrad_bn_dx\(const void\* g,", header)
    assert "#define MRLA_ABI_VERSION 5" in header


def test_query():
    from mrla_amd import _lib as L
    lib = L.load()
    q = lib.mrla_conv1x1_wgrad_bn_dx_supported
    for m in (1000, 8192, 802816):
        for dt in (L.BF16, L.F16):
            assert q(m, 64, 256, dt) == 1, (m, dt)
            assert lib.mrla_conv1x1_wgrad_bn_supported(m, 64, 256, dt) == 1
            plan = L.conv1x1_wgrad_plan(m, 64, 256, dt)
            assert (plan[2], plan[3], plan[5]) == (256, 64, 1)          # ONE 256 x 64 tile
            for k, n in ((128, 512), (256, 64), (64, 64), (64, 128)):
                assert q(m, k, n, dt) == L.EUNSUPPORTED, (m, k, n, dt)
        assert q(m, 64, 256, L.F32) == L.EUNSUPPORTED
    assert q(1 << 24, 64, 256, L.BF16) == L.EUNSUPPORTED and q((1 << 24) + 5, 64, 256, L.F16) == L.EUNSUPPORTED
    assert q(0, 64, 256, L.BF16) == L.EINVAL


def test_launch_refuses_what_the_query_refuses_and_validates_its_arguments():
    from mrla_amd import _lib as L
    lib = L.load()
    one, two, three, four = (ctypes.c_void_p(16 * i) for i in (1, 2, 3, 4))
    odd = ctypes.c_void_p(24)

    def call(dtype, dw_dtype, m=64, k=64, n=256, g=one, xb=two, sc=one, sh=one, cb=one, x=three, wt=one, dx=four, part=one,
             dw=one):
        return lib.mrla_conv1x1_wgrad_bn_dx(g, xb, sc, sh, cb, 1, x, wt, dx, part, dw, m, k, n, dtype, dw_dtype, None)
    # nothing is launched in any of these
    for k, n in ((128, 512), (256, 64), (64, 64), (64, 128)):
        assert call(L.BF16, L.F32, m=4096, k=k, n=n) == L.EUNSUPPORTED, (k, n)
    assert call(L.F16, L.F32, m=1 << 24) == L.EUNSUPPORTED
    assert call(L.F32, L.F32) == L.EUNSUPPORTED
    assert call(L.BF16, L.F32, m=0) == L.EINVAL
    assert call(L.BF16, L.F16) == L.EINVAL and call(L.F16, L.BF16) == L.EINVAL          # mixed 16-bit dw_dtype
    for name in ("g", "xb", "sc", "sh", "cb", "x", "wt", "dx", "part", "dw"):
        assert call(L.BF16, L.F32, **{name: None}) == L.EINVAL, name
    # the lanes read sc, sh, cb and the rows of wt as 16-byte vectors and store 16-byte pieces of dx
    for name in ("sc", "sh", "cb", "wt", "dx"):
        assert call(L.BF16, L.F32, **{name: odd}) == L.EINVAL, name
        assert call(L.F16, L.F32, **{name: odd}) == L.EINVAL, name
    # dx is written while g, xb and x are still being read
    assert call(L.BF16, L.F32, dx=one) == L.EINVAL and call(L.BF16, L.F32, dx=two) == L.EINVAL
    assert call(L.BF16, L.F32, dx=three) == L.EINVAL


pytestmark_hipcc = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")


@pytest.fixture(scope="module")
def kernels():
    return kr.kernel_resources("conv1x1_wgrad.hip")


@pytestmark_hipcc
def test_the_new_instances_exist_and_fit(kernels):
    found = {}
    for k in kernels:
        m = re.search(r"conv1x1_wgrad_bn_dx(_f16)?_kernelILi4EEE", k["mangled"])
        if m:
            found[m.group(1) is not None] = k
    assert set(found) == {False, True}, sorted(k["mangled"] for k in kernels)
    for f16, k in found.items():
        assert k["scratch"] == 0, f"f16={f16}: {k['scratch']} bytes of scratch per lane"
        assert k["waves"] >= 1, f"f16={f16}: {k['vgprs']} VGPRs + {k['agprs']} AGPRs do not fit one wave per SIMD"
        assert k["vgprs"] + k["agprs"] <= 512, (f16, k["vgprs"], k["agprs"])


@pytestmark_hipcc
def test_plain_and_bn_instances_keep_the_parents_figures(kernels):
    seen = set()
    for k in kernels:
        m = re.search(r"conv1x1_wgrad(_bn)?(_f16)?_kernelILi(\d+)ELi(\d+)ELi4ELi32EEE", k["mangled"])
        if not m:
            continue
        bn, f16, tile = m.group(1) is not None, m.group(2) is not None, (int(m.group(3)), int(m.group(4)))
        want = (BN_F16 if f16 else BN_BF16)[tile] if bn else PLAIN[tile]
        assert (k["vgprs"], k["agprs"], k["waves"]) == want and k["scratch"] == 0, ((bn, f16, tile), k)
        seen.add((bn, f16, tile))
    assert seen == {(bn, f16, t) for bn in (False, True) for f16 in (False, True) for t in TILES}
