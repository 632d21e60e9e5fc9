"""Compiler- and host-side gates on the 1x1 GEMMs with an eval-mode BatchNorm (+ReLU) folded into their store
(mrla_conv1x1_fwd_affine; resnet_mrla_light.py:93-94 and :196-199 under model.eval()).  Needs hipcc for the compiler gate,
never a GPU.

  * the two exports are additive: both are declared and bound, the ABI version stays 5 and the signatures of the entry points
    beside them do not move;
  * the host decides what it can before anything is launched: which shapes and dtypes are taken, a `relu` outside {0, 1}
    and an empty problem;
  * every *_affine_kernel instance is launched in place of the plain forward instance (no moment records, no addend) of the
    same tile on the same grid with the same LDS: it may not spill, nor compile to fewer waves per SIMD than that twin, and
    the narrow ones keep the waves conv1x1_geo() plans with -- 2 for eight waves per workgroup, 3 for four."""
import functools
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

needs_hipcc = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")


def test_the_new_exports_are_additive():
    from mrla_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mrla_hip.h")).read()
    for name in ("mrla_conv1x1_fwd_affine_supported", "mrla_conv1x1_fwd_affine"):
        assert name in L.SIGNATURES and re.search(r"\bint " + name + r"\(", header), name
    P, I = L._P, L._I
    assert L.SIGNATURES["mrla_conv1x1_fwd_affine_supported"] == [I] * 4
    assert L.SIGNATURES["mrla_conv1x1_fwd_affine"] == [P, P, P, P, I, P, I, I, I, I, P]
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5
    assert L.load().mrla_abi_version() == 5
    # the entry points beside them, as they were
    assert L.SIGNATURES["mrla_conv1x1_fwd"] == [P, P, P, P, I, I, I, I, P]
    assert L.SIGNATURES["mrla_conv1x1_fwd_add"] == [P, P, P, P, I, I, I, I, P]
    assert L.SIGNATURES["mrla_conv1x1_fwd_addend"] == [P, P, P, P] + [I] * 9 + [P]


def test_host_side_answers():
    from mrla_amd import _lib as L
    lib = L.load()
    for dt in (L.BF16, L.F16):
        for m, k, n in ((98, 64, 64), (98, 64, 256), (98, 512, 128), (20300, 1024, 512)):     # narrow, wide, K-streaming x 2
            assert lib.mrla_conv1x1_fwd_affine_supported(m, k, n, dt) == 1, (m, k, n, dt)
            assert lib.mrla_conv1x1_rows(m, k, n, dt) > 0
        assert lib.mrla_conv1x1_fwd_affine_supported(98, 96, 256, dt) == L.EUNSUPPORTED        # a k no GEMM takes
    assert lib.mrla_conv1x1_fwd_affine_supported(98, 64, 64, L.F32) == L.EUNSUPPORTED
    # decided on the host, nothing launched (dummy pointers, as tests/test_shortcut_addend_cpu.py passes them)
    p = 16
    assert lib.mrla_conv1x1_fwd_affine(p, p, p, p, 2, p, 98, 64, 64, L.BF16, None) == L.EINVAL      # relu outside {0, 1}
    assert lib.mrla_conv1x1_fwd_affine(p, p, p, p, -1, p, 98, 64, 64, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_affine(p, p, p, p, 1, p, 0, 64, 64, L.BF16, None) == L.EINVAL       # m = 0
    assert lib.mrla_conv1x1_fwd_affine(p, p, None, p, 1, p, 98, 64, 64, L.BF16, None) == L.EINVAL   # a null pointer
    assert lib.mrla_conv1x1_fwd_affine(p, p, p, p, 1, p, 98, 96, 256, L.BF16, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_fwd_affine(p, p, p, p, 1, p, 98, 64, 64, L.F32, None) == L.EUNSUPPORTED


@functools.lru_cache(maxsize=None)
def _resources(src):
    return kr.kernel_resources(src)            # (one compilation per source file for the whole module)


def _instances(src, pattern):
    out = {}
    for k in _resources(src):
        m = re.search(pattern, k["mangled"])
        if m:
            out[tuple(int(g) for g in m.groups())] = k
    return out


@needs_hipcc
@pytest.mark.parametrize("f16", ["", "f16_"], ids=["bf16", "fp16"])
def test_narrow_affine_instances(f16):
    aff = _instances("conv1x1.hip", r"conv1x1_fwd_" + f16 + r"affine_kernelILi(\d+)ELi(\d+)E")          # <KS, NW>
    plain = _instances("conv1x1.hip", r"conv1x1_fwd_" + f16 + r"kernelILi(\d+)ELb0ELi(\d+)E")           # <KS, MOM = 0, NW>
    # launch_conv1x1_affine: K = 64 / 128 with four or eight waves, K = 256 with eight -- as launch_conv1x1_fwd
    assert set(aff) == set(plain) == {(4, 4), (4, 8), (8, 4), (8, 8), (16, 8)}, (sorted(aff), sorted(plain))
    for (ks, nw), k in sorted(aff.items()):
        assert k["scratch"] == 0, f"<{ks}, {nw}>: {k['scratch']} bytes of scratch per lane"
        need = 2 if nw == 8 else 3
        assert k["waves"] >= need, f"<{ks}, {nw}>: {k['waves']} waves / SIMD ({k['vgprs']} VGPRs + {k['agprs']} AGPRs), needs {need}"
        assert k["waves"] >= plain[(ks, nw)]["waves"], (ks, nw, k["waves"], plain[(ks, nw)]["waves"])


@needs_hipcc
@pytest.mark.parametrize("src, affine, plain, count", [
    ("conv1x1_wide.hip", r"conv1x1_wide_{}affine_kernelILi(\d+)E", r"conv1x1_wide_{}kernelILi(\d+)ELb0ELb0ELb0E", 3),
    ("conv1x1_kstream.hip", r"conv1x1_kstream_{}affine_kernelILi(\d+)ELi(\d+)E", r"conv1x1_kstream_{}kernelILi(\d+)ELi(\d+)ELb0ELb0E", 4),
    ("conv1x1_kstream.hip", r"conv1x1_kstream256_{}affine_kernelE()", r"conv1x1_kstream256_{}kernelILb0ELb0E()", 1),
], ids=["wide", "kstream", "kstream256"])
@pytest.mark.parametrize("f16", ["", "f16_"], ids=["bf16", "fp16"])
def test_wide_and_kstream_affine_instances_match_their_twins(src, affine, plain, count, f16):
    res = _resources(src)

    def pick(pattern):
        out = {}
        for k in res:
            m = re.search(pattern.format(f16), k["mangled"])
            if m:
                out[m.groups()] = k
        return out
    aff, twin = pick(affine), pick(plain)
    assert len(aff) == count and set(aff) == set(twin), (sorted(aff), sorted(twin))
    for shape, k in aff.items():
        assert k["scratch"] == 0, (shape, k["mangled"], k["scratch"])
        assert k["waves"] >= twin[shape]["waves"], (shape, k["waves"], twin[shape]["waves"], k["vgprs"], k["agprs"])
