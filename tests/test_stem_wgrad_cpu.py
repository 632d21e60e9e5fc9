"""Host side and compiler side of mrla_stem_conv_wgrad (mrla_amd/csrc/stem_wgrad.hip) and of its switch in the Python layer.
Needs the built library and, for the resource figures, hipcc -- not a GPU.

  * the three symbols are exported, declared and bound, and the ABI version is still 5;
  * argument validation: every MRLA_EINVAL / MRLA_EUNSUPPORTED case of the header's contract, decided before any launch, and
    the queries answering the launch's codes; the size bound at and just below; n = 96; odd widths are SERVED, as the
    kernel's header says;
  * the planner: splits = rows of part, the splits' ranges of output rows tile all output rows exactly once, none empty, and
    the LDS of a workgroup stays under the kernel's stated 64 KB;
  * no scratch in any compiled instance;
  * the switch is off by default, and off means conv(x) itself; stem_conv_applies refuses CPU tensors and every excluded
    configuration."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

NAMES = ("mrla_stem_conv_wgrad_rows", "mrla_stem_conv_wgrad_plan", "mrla_stem_conv_wgrad")
LDS_CAP = 64 * 1024          # kSwLdsCap of stem_wgrad.hip


def test_symbols_are_exported_declared_and_bound():
    from mrla_amd import _lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "mrla_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert "#define MRLA_ABI_VERSION 5" in header and L.ABI_VERSION == 5 and lib.mrla_abi_version() == 5
    assert callable(L.stem_conv_wgrad_plan)


def test_queries_validate_their_arguments():
    from mrla_amd import _lib as L
    lib = L.load()
    rows, plan = lib.mrla_stem_conv_wgrad_rows, lib.mrla_stem_conv_wgrad_plan
    out = (ctypes.c_int * 7)()
    po = ctypes.cast(out, ctypes.c_void_p)
    good = (8, 64, 64, 64)
    for dt in (L.BF16, L.F16):
        assert rows(*good, dt) > 0 and plan(*good, dt, po) == L.OK and out[2] == rows(*good, dt)
        assert rows(8, 64, 5, 7, dt) > 0 and rows(1, 64, 3, 257, dt) > 0 and rows(2, 128, 1, 1, dt) > 0     # odd widths are served
    cases = [((8, 96, 64, 64), L.EUNSUPPORTED), ((8, 32, 64, 64), L.EUNSUPPORTED),        # n % 64
             ((256, 64, 256, 256), L.EUNSUPPORTED),                                       # b*h*w*max(3, n)*2 = 2^31
             ((128, 128, 256, 256), L.EUNSUPPORTED),                                      # ... on n
             ((0, 64, 64, 64), L.EINVAL), ((8, 0, 64, 64), L.EINVAL), ((8, -64, 64, 64), L.EINVAL),
             ((8, 64, 0, 64), L.EINVAL), ((8, 64, 64, -1), L.EINVAL)]
    for args, code in cases:
        for dt in (L.BF16, L.F16):
            assert rows(*args, dt) == code, (args, dt)
            assert plan(*args, dt, po) == code, (args, dt)
    assert rows(255, 64, 256, 256, L.BF16) > 0 and rows(127, 128, 256, 256, L.F16) > 0       # just below the bound
    assert rows(*good, L.F32) == L.EUNSUPPORTED and plan(*good, L.F32, po) == L.EUNSUPPORTED
    assert rows(*good, 7) == L.EINVAL and plan(*good, 7, po) == L.EINVAL     # a dtype code that is none
    assert plan(*good, L.BF16, None) == L.EINVAL                             # null out


def test_launch_validates_its_arguments_before_launching():
    from mrla_amd import _lib as L
    lib = L.load()
    one, two, three, four = (ctypes.c_void_p(16 * i) for i in (1, 2, 3, 4))
    odd = ctypes.c_void_p(24)

    def call(dtype, dw_dtype, shape=(8, 64, 64, 64), dy=one, x=two, part=three, dw=four):
        return lib.mrla_stem_conv_wgrad(dy, x, part, dw, *shape, dtype, dw_dtype, None)
    # nothing is launched in any of these
    for name in ("dy", "x", "part", "dw"):
        assert call(L.BF16, L.F32, **{name: None}) == L.EINVAL, name
        assert call(L.BF16, L.F32, **{name: odd}) == L.EINVAL, name
        assert call(L.F16, L.F16, **{name: odd}) == L.EINVAL, name
    assert call(L.BF16, L.F16) == L.EINVAL and call(L.F16, L.BF16) == L.EINVAL      # a 16-bit dw_dtype other than dtype
    assert call(L.BF16, 7) == L.EINVAL and call(7, L.F32) == L.EINVAL
    assert call(L.F32, L.F32) == L.EUNSUPPORTED
    for shape in ((8, 96, 64, 64), (256, 64, 256, 256)):
        assert call(L.BF16, L.F32, shape=shape) == L.EUNSUPPORTED, shape
        assert call(L.F16, L.F16, shape=shape) == L.EUNSUPPORTED, shape
    for shape in ((0, 64, 64, 64), (8, 64, 64, 0), (8, 64, -3, 64), (8, -64, 64, 64)):
        assert call(L.BF16, L.F32, shape=shape) == L.EINVAL, shape


def test_rows_equal_the_plans_splits():
    from mrla_amd import _lib as L
    lib = L.load()
    for b, n, h, w in ((1, 64, 1, 1), (1, 64, 5, 7), (2, 64, 9, 6), (3, 128, 14, 10), (5, 64, 40, 40), (256, 64, 224, 224),
                       (64, 64, 224, 224), (2, 64, 800, 1344), (1, 64, 3, 257), (1, 192, 1, 4001)):
        for dt in (L.BF16, L.F16):
            plan = L.stem_conv_wgrad_plan(b, n, h, w, dt)
            assert plan is not None and plan[2] == lib.mrla_stem_conv_wgrad_rows(b, n, h, w, dt) > 0, (b, n, h, w)
            assert plan[0] == 64 and plan[3] == -(-((w - 1) // 2 + 1) // plan[5])


def test_the_splits_tile_the_output_rows_exactly_once_and_the_lds_stays_under_the_cap():
    """b in {1, 2, 8, 256}, n = 64, maps 1 .. 230.  Split i takes the output rows [i * per, min(total, (i + 1) * per)):
    together every row once, none empty."""
    from mrla_amd import _lib as L
    worst = 0
    for b in (1, 2, 8, 256):
        for hw in range(1, 231):
            tn, per, splits, nseg, lds, ws, rmax = L.stem_conv_wgrad_plan(b, 64, hw, hw, L.BF16)
            ho = wo = (hw - 1) // 2 + 1
            total = b * ho
            assert tn == 64 and per >= 1 and splits >= 1 and nseg >= 1 and 1 <= rmax <= ho and 1 <= ws <= wo
            assert (splits - 1) * per < total <= splits * per, (b, hw, per, splits)      # no gap, no empty split
            assert (nseg - 1) * ws < wo <= nseg * ws
            assert 0 < lds <= LDS_CAP, (b, hw, lds)
            worst = max(worst, lds)
    for w in (255, 256, 257, 511, 1344, 4001):                                  # ... and rows cut into column segments
        lds = L.stem_conv_wgrad_plan(1, 64, 3, w, L.F16)[4]
        assert 0 < lds <= LDS_CAP, (w, lds)
        worst = max(worst, lds)
    assert worst > LDS_CAP // 2          # (the cap is the kernel's, not a number far above what it uses)


@pytest.mark.skipif(kr.find_hipcc() is None, reason="hipcc not found: the resource figures come from the compiler")
def test_no_instance_of_the_new_file_uses_scratch():
    kernels = kr.kernel_resources("stem_wgrad.hip")
    main = [k for k in kernels if "stem_wgrad_kernel" in k["mangled"]]
    assert len(main) == 2 and sum("split_sum_kernel" in k["mangled"] for k in kernels) == 3      # bf16 / fp16; three dw types
    bad = {k["mangled"]: k["scratch"] for k in kernels if k["scratch"] != 0}
    assert not bad, f"instances with scratch (bytes per lane): {bad}"
    for k in main:           # __launch_bounds__(256, 2): the planner's two workgroups per CU
        assert k["waves"] >= 2, (k["mangled"], k["vgprs"], k["agprs"])


def _conv(cin=3, cout=64, **kw):
    args = dict(kernel_size=7, stride=2, padding=3, bias=False)
    args.update(kw)
    return torch.nn.Conv2d(cin, cout, **args)


def test_the_switch_is_off_by_default_and_off_means_the_module_itself():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert Fm.STEM_WGRAD is False
    conv = _conv()
    x = torch.randn(2, 3, 10, 10, requires_grad=True)
    y = Fm.stem_conv(x, conv)
    assert torch.equal(y, conv(x)) and type(y.grad_fn).__name__ == type(conv(x).grad_fn).__name__
    with mrla_amd.stem_wgrad():
        assert Fm.STEM_WGRAD is True and Fm.CONV3X3_WGRAD is False
        with mrla_amd.stem_wgrad(False):
            assert Fm.STEM_WGRAD is False
        assert Fm.STEM_WGRAD is True
        y = Fm.stem_conv(x, conv)                                 # a CPU tensor: not eligible, the module itself
        assert torch.equal(y, conv(x)) and type(y.grad_fn).__name__ == type(conv(x).grad_fn).__name__
    assert Fm.STEM_WGRAD is False
    with pytest.raises(RuntimeError):
        with mrla_amd.stem_wgrad():
            raise RuntimeError("x")
    assert Fm.STEM_WGRAD is False                                 # the previous value comes back when the block raises


def test_reproducible_gradients_sets_both_switches_and_restores_them():
    import mrla_amd
    from mrla_amd import functional as Fm
    assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (False, False)
    with mrla_amd.reproducible_gradients():
        assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (True, True)
        with mrla_amd.reproducible_gradients(False):
            assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (False, False)
        assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (True, True)
    assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (False, False)
    with mrla_amd.stem_wgrad():
        with pytest.raises(RuntimeError):
            with mrla_amd.reproducible_gradients():
                raise RuntimeError("x")
        assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (False, True)
    assert (Fm.CONV3X3_WGRAD, Fm.STEM_WGRAD) == (False, False)


def test_the_stem_of_resnet_mrlal_goes_through_stem_conv_and_is_the_module_itself_when_off():
    """With the switch off forward_features builds the graph it built before: the stem's node is the stock convolution's."""
    from mrla_amd import functional as Fm, resnet
    seen = []
    real = Fm.stem_conv

    class _Stop(Exception):          # (the layers behind the stem have no CPU path: the forward ends here)
        pass

    def spy(x, conv):
        y = real(x, conv)
        seen.append((conv, type(y.grad_fn).__name__, type(conv(x).grad_fn).__name__))
        raise _Stop
    model = resnet.resnet18_mrlal(num_classes=10)
    Fm.stem_conv = spy
    try:
        with pytest.raises(_Stop):
            model(torch.randn(1, 3, 32, 32))
    finally:
        Fm.stem_conv = real
    assert len(seen) == 1 and seen[0][0] is model.conv1 and seen[0][1] == seen[0][2]


def excluded_configurations():
    """(name, conv, make_x(device)): what stem_conv_applies refuses whatever the device -- shared with the GPU route test."""
    cl = torch.channels_last
    bf = lambda dev: torch.randn(2, 3, 12, 12, device=dev).bfloat16().contiguous(memory_format=cl)  # noqa: E731
    frozen = _conv()
    frozen.weight.requires_grad_(False)
    return [("3x3", _conv(kernel_size=3, padding=1), bf), ("stride 1", _conv(stride=1), bf), ("padding 2", _conv(padding=2), bf),
            ("bias", _conv(bias=True), bf), ("groups 3", _conv(3, 66, groups=3), bf), ("dilation 2", _conv(dilation=2, padding=6), bf),
            ("c = 4", _conv(4, 64), lambda dev: torch.randn(2, 4, 12, 12, device=dev).bfloat16().contiguous(memory_format=cl)),
            ("frozen weight", frozen, bf),
            ("fp32 outside autocast", _conv(), lambda dev: torch.randn(2, 3, 12, 12, device=dev).contiguous(memory_format=cl)),
            ("NCHW", _conv(), lambda dev: torch.randn(2, 3, 12, 12, device=dev).bfloat16())]


def test_applies_is_false_for_cpu_tensors_and_every_excluded_configuration():
    from mrla_amd import functional as Fm
    conv = _conv().bfloat16()
    x = torch.randn(2, 3, 12, 12).bfloat16().contiguous(memory_format=torch.channels_last)
    assert not Fm.stem_conv_applies(conv, x)
    for name, c, make in excluded_configurations():
        c = c if name.startswith("fp32") else c.bfloat16()
        assert not Fm.stem_conv_applies(c, make("cpu")), name
