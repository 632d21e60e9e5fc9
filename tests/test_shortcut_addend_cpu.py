"""Compiler- and host-side gates on the shortcut-addend GEMMs (mrla_conv1x1_fwd_addend).  Needs hipcc, not a GPU.

  * conv1x1_fwd_addend_kernel<KS, NW> (mrla_amd/csrc/conv1x1.hip, the narrow form with the addend on its store lanes) is
    held to what tests/test_kernel_resources_cpu.py holds its twins conv1x1_fwd_kernel<KS, false, NW> to, for the same
    reasons: no scratch (a persistent, memory-bound kernel), and the waves per SIMD conv1x1_geo() plans with -- 2 for eight
    waves per workgroup, 3 for four (K <= 128);
  * the addend instances of the wide and the K-streaming form may not spill either, nor fall below the occupancy of the
    instance without addend they are launched in place of (same grid, same LDS);
  * the two exports are additive: the ABI version and the answers of the wide form's query do not move."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

needs_hipcc = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")


@needs_hipcc
def test_narrow_addend_instances_do_not_spill_and_keep_the_planned_occupancy():
    inst = {}
    for k in kr.kernel_resources("conv1x1.hip"):
        m = re.search(r"conv1x1_fwd_addend_kernelILi(\d+)ELi(\d+)E", k["mangled"])            # <KS, NW>
        if m:
            inst[(int(m.group(1)), int(m.group(2)))] = k
    # launch_conv1x1_addend: K = 64 / 128 with four or eight waves, K = 256 with eight
    assert set(inst) == {(4, 4), (4, 8), (8, 4), (8, 8), (16, 8)}, sorted(inst)
    for (ks, nw), k in sorted(inst.items()):
        assert k["scratch"] == 0, f"<{ks}, {nw}>: {k['scratch']} bytes of scratch per lane"
        need = 2 if nw == 8 else 3
        assert k["waves"] >= need, f"<{ks}, {nw}>: {k['waves']} waves / SIMD ({k['vgprs']} VGPRs + {k['agprs']} AGPRs), needs {need}"


@needs_hipcc
@pytest.mark.parametrize("src, pattern", [
    ("conv1x1_wide.hip", r"conv1x1_wide_kernelILi(\d+)ELb0ELb([01])ELb([01])E"),               # <KS, MOM = 0, ADD, SP>
    ("conv1x1_kstream.hip", r"conv1x1_kstream_kernelILi(\d+)ELi(\d+)ELb0ELb([01])E"),           # <WN, PB, MOM = 0, ADD>
    ("conv1x1_kstream.hip", r"conv1x1_kstream256_kernelILb0ELb([01])E"),                        # <MOM = 0, ADD>
])
def test_wide_and_kstream_addend_instances_match_their_twins(src, pattern):
    wide = "wide" in src
    groups = {}                                 # shape parameters -> {addend flags -> figures}
    for k in kr.kernel_resources(src):
        m = re.search(pattern, k["mangled"])
        if m:
            g = m.groups()
            shape, flags = (g[:1], g[1] + g[2]) if wide else (g[:-1], g[-1])
            groups.setdefault(shape, {})[flags] = k
    assert groups
    with_addend, twin = ("11", "10") if wide else ("1", "0")     # wide: the compact form against the full-size one
    for shape, g in groups.items():
        assert set(g) == ({"00", "10", "11"} if wide else {"0", "1"}), (shape, sorted(g))
        for k in g.values():
            assert k["scratch"] == 0, (shape, k["mangled"], k["scratch"])
        assert g[with_addend]["waves"] >= g[twin]["waves"], (shape, g[with_addend]["waves"], g[twin]["waves"])


def test_the_new_exports_are_additive():
    from mrla_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mrla_hip.h")).read()
    for name in ("mrla_conv1x1_addend_supported", "mrla_conv1x1_fwd_addend"):
        assert name in L.SIGNATURES and re.search(r"\bint " + name + r"\(", header), name
    assert len(L.SIGNATURES["mrla_conv1x1_addend_supported"]) == 6 and len(L.SIGNATURES["mrla_conv1x1_fwd_addend"]) == 14
    assert L.SIGNATURES["mrla_conv1x1_fwd_add"] == [L._P, L._P, L._P, L._P, L._I, L._I, L._I, L._I, L._P]
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5
    lib = L.load()
    assert lib.mrla_abi_version() == 5
    # host-side answers (no GPU touched): geometry is validated before anything is launched
    p = 16
    assert lib.mrla_conv1x1_fwd_addend(p, p, p, p, 100, 64, 256, 2, 7, 7, 2, 2, L.BF16, None) == L.EINVAL      # b*h*w != m
    assert lib.mrla_conv1x1_fwd_addend(p, p, p, p, 98, 64, 256, 2, 7, 7, 2, 0, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_addend_supported(98, 64, 256, 2, 2, L.BF16) == 1
    assert lib.mrla_conv1x1_addend_supported(98, 64, 64, 1, 1, L.BF16) == 1
    assert lib.mrla_conv1x1_addend_supported(98, 512, 2048, 1, 1, L.BF16) == 1
    assert lib.mrla_conv1x1_addend_supported(98, 96, 256, 2, 2, L.BF16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_add_supported(98, 64, 64, L.BF16) == L.EUNSUPPORTED                               # as before
    assert lib.mrla_conv1x1_add_supported(98, 512, 2048, L.BF16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_add_supported(98, 64, 256, L.BF16) == 1
