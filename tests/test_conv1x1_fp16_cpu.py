"""Host- and compiler-side gates on the fp16 forms of the 1x1-convolution GEMMs.  Needs hipcc for the second half, no GPU.

  * every mrla_conv1x1_* query answers for MRLA_F16 exactly what it answers for MRLA_BF16 (same planners, grids, record
    rows), MRLA_F32 stays MRLA_EUNSUPPORTED, a 16-bit dw_dtype other than the operands' is MRLA_EINVAL, and null pointers
    are refused before anything is launched;
  * the widening is additive: ABI 5, and mrla_weight_bank_refresh_dt is declared, exported and bound;
  * every fp16 kernel instance of conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip (and the weight
    bank's cast) has a bf16 twin with the same shape parameters and flags, carries no scratch and reaches at least the
    twin's waves per SIMD; the narrow fp16 instances meet the occupancy conv1x1_geo() plans with (2 for eight waves per
    workgroup, 3 for four, K <= 128: tests/test_kernel_resources_cpu.py)."""
import concurrent.futures
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

needs_hipcc = pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")

# (m, k, n): one shape per planner branch, then the unsupported ones
SHAPES = [
    (3136, 64, 64), (48, 64, 64), (1, 256, 64), (6272, 128, 192), (6272, 256, 128),          # narrow: 4 / 8 waves, ragged, one pixel
    (6272, 64, 256), (162, 128, 256), (784, 256, 1024), (1, 256, 256),                       # wide
    (64, 512, 128), (64, 544, 128), (12544, 512, 128), (12544, 512, 256), (64, 1024, 256),   # K-streaming: pb = 1 / 2
    (46081, 1024, 256), (100352, 2048, 512),                                                 # ... and its 256 x 256 tile
    (3136, 192, 320), (98, 2048, 512), (33, 64, 64),                                         # weight gradient only / tile classes
    (64, 96, 64), (64, 64, 96), (64, 520, 128), (64, 512, 64),                               # k = 96, n = 96, k = 520, n % 128
    (1 << 24, 128, 64), (1 << 22, 256, 64), (1 << 23, 64, 256),                              # m * max(n, k) * 2 >= 2^31
]


def _answers(lib, L, m, k, n, dt):
    plan, plan_add, wplan = (ctypes.c_int * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int * 6)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)                                            # noqa: E731
    rc = (lib.mrla_conv1x1_rows(m, k, n, dt), lib.mrla_conv1x1_plan(m, k, n, dt, 0, P(plan)),
          lib.mrla_conv1x1_plan(m, k, n, dt, 1, P(plan_add)), lib.mrla_conv1x1_wgrad_rows(m, k, n, dt),
          lib.mrla_conv1x1_wgrad_plan(m, k, n, dt, P(wplan)), lib.mrla_conv1x1_add_supported(m, k, n, dt),
          lib.mrla_conv1x1_addend_supported(m, k, n, 1, 1, dt), lib.mrla_conv1x1_addend_supported(m, k, n, 2, 2, dt))
    return rc + (tuple(plan) if rc[1] == L.OK else None, tuple(plan_add) if rc[2] == L.OK else None,
                 tuple(wplan) if rc[4] == L.OK else None)


def test_fp16_queries_answer_as_the_bf16_ones():
    from mrla_amd import _lib as L
    lib = L.load()
    seen = set()
    for m, k, n in SHAPES:
        a16, ab = _answers(lib, L, m, k, n, L.F16), _answers(lib, L, m, k, n, L.BF16)
        assert a16 == ab, ((m, k, n), a16, ab)
        a32 = _answers(lib, L, m, k, n, L.F32)
        assert all(rc == L.EUNSUPPORTED for rc in a32[:8]), ((m, k, n), a32)
        seen.add((a16[0] > 0, a16[3] > 0))
        assert L.conv1x1_plan(m, k, n, dtype=L.F16) == L.conv1x1_plan(m, k, n) == a16[8]
        assert L.conv1x1_wgrad_plan(m, k, n, dtype=L.F16) == L.conv1x1_wgrad_plan(m, k, n) == a16[10]
    assert {(True, True), (False, True), (False, False)} <= seen              # the table holds taken and refused shapes
    # the branches the table is meant to reach, read off the fp16 answers
    assert lib.mrla_conv1x1_rows(64, 96, 64, L.F16) == L.EUNSUPPORTED and lib.mrla_conv1x1_rows(64, 64, 96, L.F16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_rows(64, 520, 128, L.F16) == L.EUNSUPPORTED and lib.mrla_conv1x1_rows(64, 544, 128, L.F16) == 1
    assert lib.mrla_conv1x1_wgrad_rows(1 << 24, 128, 64, L.F16) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_addend_supported(1 << 22, 256, 64, 1, 1, L.F16) == L.EUNSUPPORTED
    assert L.conv1x1_plan(46081, 1024, 256, dtype=L.F16)[1] == 4 and L.conv1x1_plan(64, 1024, 256, dtype=L.F16)[1] == 3
    assert lib.mrla_conv1x1_rows(0, 64, 64, L.F16) == L.EINVAL


def test_fp16_entry_points_validate_before_they_launch():
    from mrla_amd import _lib as L
    lib = L.load()
    p = 16                               # (a non-null pointer that is never dereferenced: the checks below fail first)
    assert lib.mrla_conv1x1_fwd(None, None, None, None, 64, 1024, 256, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd(p, p, None, None, 64, 64, 64, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_add(p, p, None, p, 64, 64, 256, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_addend(p, p, None, p, 98, 64, 256, 2, 7, 7, 2, 2, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_fwd_addend(p, p, p, p, 100, 64, 256, 2, 7, 7, 2, 2, L.F16, None) == L.EINVAL      # b*h*w != m
    assert lib.mrla_conv1x1_wgrad(None, None, None, None, 64, 64, 64, L.F16, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_wgrad(p, p, p, None, 64, 64, 64, L.F16, L.F32, None) == L.EINVAL
    # dw is of the operands' type or fp32
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 64, 64, L.F16, L.BF16, None) == L.EINVAL
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 64, 64, L.BF16, L.F16, None) == L.EINVAL
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 64, 64, L.F16, 7, None) == L.EINVAL
    # unsupported shapes and fp32 operands are reported, not run
    assert lib.mrla_conv1x1_fwd(p, p, p, None, 64, 96, 64, L.F16, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_fwd(p, p, p, None, 64, 64, 64, L.F32, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_fwd_add(p, p, p, p, 64, 64, 64, L.F16, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_fwd_addend(p, p, p, p, 98, 96, 256, 2, 7, 7, 2, 2, L.F16, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 96, 64, L.F16, L.F16, None) == L.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad(p, p, p, p, 64, 64, 64, L.F32, L.F32, None) == L.EUNSUPPORTED
    # the weight bank's additive entry point
    assert lib.mrla_weight_bank_refresh_dt(None, 1, 1, L.F16, None) == L.EINVAL
    assert lib.mrla_weight_bank_refresh_dt(p, 0, 1, L.F16, None) == L.EINVAL
    assert lib.mrla_weight_bank_refresh_dt(p, 1, 1, 7, None) == L.EINVAL
    assert lib.mrla_weight_bank_refresh_dt(p, 1, 1, L.F32, None) == L.EUNSUPPORTED


def test_the_widening_is_additive():
    from mrla_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "mrla_hip.h")).read()
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and L.load().mrla_abi_version() == 5
    assert re.search(r"^int mrla_weight_bank_refresh_dt\(const void\* table, int entries, int max_tiles, int dtype, void\* stream\);",
                     header, flags=re.M)
    assert L.SIGNATURES["mrla_weight_bank_refresh_dt"] == [L._P, L._I, L._I, L._I, L._P]
    assert L.SIGNATURES["mrla_weight_bank_refresh"] == [L._P, L._I, L._I, L._P]              # as before: bf16
    assert hasattr(L.load(), "mrla_weight_bank_refresh_dt")


# ---- compiler gates --------------------------------------------------------------------------------------------------
FILES = ("conv1x1.hip", "conv1x1_wide.hip", "conv1x1_kstream.hip", "conv1x1_wgrad.hip", "weight_bank.hip")
# kernel name, then the template list: integers and flags, or the reduce kernel's output type
_NAME = re.compile(r"\d+((?:conv1x1|weight_bank)_[a-z0-9_]*?kernel)(I(?:L[ib]\d+E)+E|IDF16bE|IfE)?")


@pytest.fixture(scope="module")
def kernels():
    """{file: {(kernel name without _f16, template list): {"bf16": figures, "f16": figures}}}"""
    with concurrent.futures.ThreadPoolExecutor(len(FILES)) as pool:
        per_file = list(pool.map(kr.kernel_resources, FILES))
    out = {}
    for src, ks in zip(FILES, per_file):
        pairs = out.setdefault(src, {})
        for k in ks:
            m = _NAME.search(k["mangled"])
            assert m, k["mangled"]
            name, tpl = m.group(1), m.group(2) or ""
            if tpl == "IfE":
                continue                              # the reduce kernel's fp32 output: shared by both element types
            if tpl == "IDF16bE":
                tpl = ""                              # conv1x1_wgrad_reduce_kernel<bf16>, twin of ..._reduce_f16_kernel
            half = "_f16" in name
            slot = pairs.setdefault((name.replace("_f16", ""), tpl), {})
            assert ("f16" if half else "bf16") not in slot, k["mangled"]
            slot["f16" if half else "bf16"] = k
    return out


@needs_hipcc
@pytest.mark.parametrize("src", FILES)
def test_every_fp16_instance_has_a_twin_no_scratch_and_the_twins_occupancy(kernels, src):
    pairs = kernels[src]
    assert pairs
    for key, g in sorted(pairs.items()):
        assert set(g) == {"bf16", "f16"}, (key, sorted(g))          # an fp16 instance of every launched instance, no more
        h, b = g["f16"], g["bf16"]
        assert h["scratch"] == 0, (key, h["scratch"])
        assert h["waves"] >= b["waves"], f"{key}: fp16 {h['waves']} waves / SIMD ({h['vgprs']} VGPRs + {h['agprs']} AGPRs), bf16 {b['waves']}"
        assert h["lds"] == b["lds"], key


@needs_hipcc
def test_narrow_fp16_instances_keep_the_planned_occupancy(kernels):
    fwd, addend = {}, {}
    for (name, tpl), g in kernels["conv1x1.hip"].items():
        nums = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", tpl))
        if name == "conv1x1_fwd_kernel":
            fwd[nums] = g["f16"]                       # <KS, MOM, NW>
        elif name == "conv1x1_fwd_addend_kernel":
            addend[nums] = g["f16"]                    # <KS, NW>
    assert set(fwd) == {(ks, mom, nw) for ks in (4, 8) for mom in (0, 1) for nw in (4, 8)} | {(16, 0, 8), (16, 1, 8)}
    assert set(addend) == {(4, 4), (4, 8), (8, 4), (8, 8), (16, 8)}
    for key, k in sorted(list(fwd.items()) + list(addend.items())):
        ks, nw = key[0], key[-1]
        assert "f16" in k["mangled"] and "DF16_" in k["mangled"] and "DF16b" not in k["mangled"], k["mangled"]
        if nw == 4 and ks > 8:
            continue                                   # never launched: conv1x1_geo() takes eight waves above K = 128
        need = 2 if nw == 8 else 3
        assert k["waves"] >= need, f"{key}: {k['waves']} waves / SIMD ({k['vgprs']} VGPRs + {k['agprs']} AGPRs), needs {need}"
