"""Compiler-side gate on the narrow 1x1 GEMM (mrla_amd/csrc/conv1x1.hip): no instance of conv1x1_fwd_kernel may spill,
and each must reach the occupancy its launch bounds and its planner assume.  Needs hipcc, not a GPU.

The bounds are conditions of the design, not measurements:
  * scratch = 0: the kernel is persistent over pixel blocks, so a spill is scratch traffic inside the block loop of a
    kernel that is limited by memory (the K = 256 instance with the moment epilogue once carried 372 bytes per lane and
    took three times as long as its twin without the epilogue);
  * NW = 8 (512 lanes, __launch_bounds__ caps a lane at 256 registers): >= 2 waves per SIMD = one whole workgroup per CU;
  * NW = 4: conv1x1_geo() launches these for K <= 128 with `want = 256 * 3` workgroups, three per CU, which is
    3 * 4 waves / 4 SIMDs = 3 waves per SIMD.
Only this one file is compiled (device side only); scripts/kernel_resources.py prints the same figures for every kernel."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")


@pytest.fixture(scope="module")
def instances():
    out = {}
    for k in kr.kernel_resources("conv1x1.hip"):
        m = re.search(r"conv1x1_fwd_kernelILi(\d+)ELb([01])ELi(\d+)E", k["mangled"])      # <KS, MOM, NW>
        if m:
            out[(int(m.group(1)), m.group(2) == "1", int(m.group(3)))] = k
    return out


def test_every_launched_instance_is_compiled(instances):
    # launch_conv1x1_fwd: K = 64 / 128 with four or eight waves, K = 256 with eight, each with and without the epilogue
    want = {(ks, mom, nw) for ks in (4, 8) for mom in (True, False) for nw in (4, 8)} | {(16, True, 8), (16, False, 8)}
    assert want <= set(instances), sorted(want - set(instances))


def test_no_instance_spills(instances):
    bad = {key: k["scratch"] for key, k in instances.items() if k["scratch"] != 0}
    assert not bad, f"conv1x1_fwd_kernel<KS, MOM, NW> instances with scratch (bytes per lane): {bad}"


def test_occupancy_the_planner_assumes(instances):
    for (ks, mom, nw), k in sorted(instances.items()):
        if nw == 4 and ks > 8:
            continue                                   # never launched: conv1x1_geo() takes eight waves above K = 128
        need = 2 if nw == 8 else 3
        assert k["waves"] >= need, f"<{ks}, {mom}, {nw}>: {k['waves']} waves / SIMD ({k['vgprs']} VGPRs + {k['agprs']} AGPRs), needs {need}"


def test_isa_diff_pairs_renamed_kernels_and_reads_the_makefile():
    """scripts/kernel_isa_diff.py: --all takes the Makefile's SRC list, and --map renames the parent's mangled names before the
    kernels are paired (a kernel that lost a template argument meets the instance it came from); two parent kernels under
    one name are an error, not a silent pairing."""
    import kernel_isa_diff as kd
    sources = kd.makefile_sources(os.path.join(ROOT, "mrla_amd", "csrc"))
    assert "light_nhwc_wide.hip" in sources and "capi.hip" in sources and len(sources) == len(set(sources))
    assert all(os.path.exists(os.path.join(ROOT, "mrla_amd", "csrc", s)) for s in sources)
    maps = [(re.compile(r"(kernelI\w+?)Lb0EEEv"), r"\1EEv")]
    parent = {"_ZN4mrla6kernelIfLb1ELb0EEEvPKT_": 1, "_ZN4mrla5otherIfEEvPKT_": 2}
    assert kd.renamed(parent, maps) == {"_ZN4mrla6kernelIfLb1EEEvPKT_": 1, "_ZN4mrla5otherIfEEvPKT_": 2}
    with pytest.raises(SystemExit):
        kd.renamed({"_ZN4mrla6kernelIfLb0EEEvPKT_": 1, "_ZN4mrla6kernelIfEEvPKT_": 2}, maps)
