"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol, the module
surface mirrors the reference's (names, ctor kwargs, state_dict keys), and the product refuses CPU tensors."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from mrla_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mrla_hip.h")).read()
    declared = set(re.findall(r"^int\s+(mrla_\w+)\s*\(", hdr, flags=re.M))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    # the version the header declares == what the library reports == what the ctypes binding was written against
    hdr_version = int(re.search(r"#define\s+MRLA_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert lib.mrla_abi_version() == hdr_version == _lib.ABI_VERSION == 5


def test_argument_validation_without_a_gpu():
    from mrla_amd import _lib
    lib = _lib.load()
    assert lib.mrla_light_wgrad_rows(0, 64, 8, 8, _lib.F32, _lib.NCHW) == _lib.EINVAL
    assert lib.mrla_light_wgrad_rows(2, 64, 8, 128, _lib.F32, _lib.NCHW) == _lib.EUNSUPPORTED
    assert lib.mrla_light_wgrad_rows(256, 256, 56, 56, _lib.BF16, _lib.NCHW) > 0
    assert lib.mrla_light_stats_fwd(None, None, None, None, 1, 32, 4, 4, _lib.F32, _lib.NCHW, 0, None) == _lib.EINVAL
    assert lib.mrla_light_gate_fwd(None, None, None, 4, None, 1, 32, 16, 32, None) == _lib.EINVAL
    # channels_last MRLA-base geometry: rows of the partial buffers, supported widths, argument checks
    assert lib.mrla_base_tile_rows(128, 1024, 14, 14, _lib.BF16, _lib.NHWC) == 128 * 28     # 7-pixel tiles
    assert lib.mrla_base_pmom_rows(128, 1024, 14, 14, _lib.BF16, _lib.NHWC) == 128 * 14     # 14-pixel tiles
    assert lib.mrla_base_tile_rows(4, 256, 56, 56, _lib.F32, _lib.NCHW) == 4
    assert lib.mrla_base_tile_rows(4, 192, 14, 14, _lib.BF16, _lib.NHWC) > 0       # DeiT widths: 240-thread workgroups
    assert lib.mrla_base_tile_rows(4, 192, 14, 14, _lib.F32, _lib.NHWC) > 0 and lib.mrla_base_tile_rows(4, 768, 14, 14, _lib.F32, _lib.NHWC) > 0
    assert lib.mrla_base_tile_rows(4, 2048, 7, 7, _lib.F32, _lib.NHWC) == _lib.EUNSUPPORTED    # 512 fp32 vectors per pixel
    assert lib.mrla_base_tile_rows(0, 256, 7, 7, _lib.BF16, _lib.NHWC) == _lib.EINVAL
    assert lib.mrla_base_pool_value_fwd(None, None, None, None, None, None, None, None, 1, 64, 4, 4, _lib.BF16, _lib.NHWC,
                                        None) == _lib.EINVAL
    assert lib.mrla_base_dv_combine(None, None, None, 1, 64, 4, 4, 16, 3, 1, 3, _lib.BF16, _lib.NHWC, None) == _lib.EINVAL
    assert lib.mrla_base_pmom_reduce(None, None, 2, 64, 3, 4, None) == _lib.EINVAL
    assert lib.mrla_light_pool_fused(None, None, None, None, None, None, 1, 64, 4, 4, _lib.BF16, _lib.NHWC, None) == _lib.EINVAL
    assert lib.mrla_bn_moment_rows(256, 256, 56, 56, _lib.NHWC) == 256 * 4 and lib.mrla_bn_moment_rows(8, 64, 7, 7, _lib.NCHW) == 8
    # the stem tail's geometry query: 6 ints for one row band; refuses what mrla_bn_pool_rows refuses, a band the shape does not
    # have and a missing result array
    import ctypes
    plan, P6 = (ctypes.c_int * 6)(), lambda a: ctypes.cast(a, ctypes.c_void_p)       # noqa: E731
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, _lib.BF16, _lib.NHWC, 7, P6(plan)) == _lib.OK and tuple(plan) == (56, 56, 8, 8, 49, 56)
    assert lib.mrla_bn_pool_rows(4, 64, 112, 112, _lib.BF16, _lib.NHWC) == 4 * 8
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, _lib.BF16, _lib.NHWC, 8, P6(plan)) == _lib.EINVAL
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, _lib.BF16, _lib.NHWC, -1, P6(plan)) == _lib.EINVAL
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, _lib.BF16, _lib.NHWC, 0, None) == _lib.EINVAL
    assert lib.mrla_bn_pool_plan(0, 64, 112, 112, _lib.BF16, _lib.NHWC, 0, P6(plan)) == _lib.EINVAL
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, 7, _lib.NHWC, 0, P6(plan)) == _lib.EINVAL
    assert lib.mrla_bn_pool_plan(4, 64, 112, 112, _lib.BF16, 2, 0, P6(plan)) == _lib.EINVAL
    for bad in ((4, 64, 112, 112, _lib.BF16, _lib.NCHW), (4, 96, 112, 112, _lib.BF16, _lib.NHWC), (4, 64, 1, 112, _lib.BF16, _lib.NHWC)):
        assert lib.mrla_bn_pool_plan(*bad, 0, P6(plan)) == lib.mrla_bn_pool_rows(*bad) == _lib.EUNSUPPORTED
    assert _lib.bn_pool_plan(1, 192, 30, 34, _lib.F16, 1) == (15, 17, 2, 5, 7, 15) and _lib.bn_pool_plan(1, 192, 30, 34, _lib.F16, 2) is None
    # 1x1-convolution GEMMs: workspace rows of the forward moments / the weight-gradient partial tiles, argument checks
    assert lib.mrla_conv1x1_rows(64, 512, 128, _lib.BF16) == 1 and lib.mrla_conv1x1_rows(64, 96, 64, _lib.BF16) == _lib.EUNSUPPORTED and lib.mrla_conv1x1_rows(48, 64, 64, _lib.BF16) > 0
    assert lib.mrla_conv1x1_wgrad_rows(256 * 56 * 56, 64, 256, _lib.BF16) == 256        # one 64x256 tile x 256 pixel ranges
    assert lib.mrla_conv1x1_wgrad_rows(256 * 7 * 7, 2048, 512, _lib.BF16) == 8          # 32 tiles of 128x256 x 8 ranges
    assert lib.mrla_conv1x1_wgrad_rows(33, 64, 64, _lib.BF16) == 2                      # two 32-pixel chunks
    assert lib.mrla_conv1x1_wgrad_rows(64, 96, 64, _lib.BF16) == _lib.EUNSUPPORTED
    assert lib.mrla_conv1x1_wgrad_rows(1 << 24, 128, 64, _lib.BF16) == _lib.EUNSUPPORTED  # 32-bit buffer offsets
    assert lib.mrla_conv1x1_wgrad(None, None, None, None, 64, 64, 64, _lib.BF16, _lib.BF16, None) == _lib.EINVAL
    # ABI 5: the tail without a stored x_t exists on the channels_last row pipeline for 16-bit activations ...
    assert lib.mrla_light_lean_supported(256, 256, 56, 56, _lib.BF16, _lib.NHWC) == 1
    assert lib.mrla_light_lean_supported(256, 256, 56, 56, _lib.F32, _lib.NHWC) == 0
    assert lib.mrla_light_lean_supported(256, 256, 56, 56, _lib.BF16, _lib.NCHW) == 0
    assert lib.mrla_light_lean_supported(256, 96, 56, 56, _lib.BF16, _lib.NHWC) == 0
    assert lib.mrla_light_stats_bwd_fused(*[None] * 8, 2, 64, 8, 8, _lib.BF16, _lib.NHWC, None) == _lib.EINVAL
    assert lib.mrla_light_apply_bwd_fused(*[None] * 16, 2, 64, 8, 8, 32, 1, _lib.BF16, _lib.NHWC, None) == _lib.EINVAL
    # ... and few, large images (a detection batch) spread an image's column strips -- and, where that does not fill the chip
    # either, its rows -- over workgroup ranges: partial rows / records = image groups x strip ranges x row ranges
    counts = lambda shape: tuple(f(*shape, _lib.BF16, _lib.NHWC) for f in (lib.mrla_light_mom_splits, lib.mrla_light_bmom_splits,      # noqa: E731
                                                                          lib.mrla_light_wgrad_rows))
    for shape, want in {(256, 256, 56, 56): (1, 1, 64), (128, 1024, 14, 14): (1, 1, 64), (2, 256, 200, 336): (6 * 8, 12 * 8, 12 * 8),
                        (2, 512, 100, 168): (3 * 8, 12 * 8, 24 * 8), (2, 1024, 50, 84): (2 * 4, 6 * 4, 12 * 4), (2, 2048, 25, 42): (2, 3, 6)}.items():
        assert counts(shape) == want, shape
    assert lib.mrla_light_lean_supported(2, 512, 100, 168, _lib.BF16, _lib.NHWC) == 0      # (the x_t-free passes walk whole images)
    assert lib.mrla_tuning_row_ranges(1) == 0                 # never cut rows: the strip ranges alone
    assert counts((2, 256, 200, 336)) == (6, 12, 12) and counts((2, 512, 100, 168)) == (3, 12, 24)
    assert lib.mrla_tuning_row_ranges(2) == 1                 # wherever an image has >= 16 rows
    assert counts((4, 256, 56, 56)) == (7, 14, 28) and counts((4, 256, 15, 56)) == (1, 2, 4)
    assert lib.mrla_tuning_row_ranges(0) == 2 and lib.mrla_tuning_row_ranges(3) == _lib.EINVAL
    assert lib.mrla_light_mom_splits(2, 96, 200, 336, _lib.BF16, _lib.NHWC) == 1          # (off the 64-lane grid: one workgroup per image)
    assert lib.mrla_light_bmom_splits(2, 256, 56, 56, _lib.BF16, _lib.NCHW) == 1 and lib.mrla_light_bmom_splits(0, 1, 1, 1, 0, 0) == _lib.EINVAL
    # the sequence entry points (ABI 4) validate like the passes they issue: the first pass's code comes back, nothing is launched
    P = [None]
    assert lib.mrla_light_tail_fwd(*P * 6, 5, *P * 6, _lib.BN_TRAIN, 0.1, 1e-5, *P * 6, 2, 64, 8, 8, 32, 1, 1, _lib.BF16, _lib.NHWC,
                                   0, None) == _lib.EINVAL
    assert lib.mrla_light_tail_bwd(*P * 5, 5, *P * 7, _lib.BN_TRAIN, *P * 5, 1, *P * 8, 2, 64, 8, 8, 32, 1, 1, _lib.BF16,
                                   _lib.NHWC, 0, None) == _lib.EINVAL
    assert lib.mrla_bn_fwd(None, None, 0, None, None, 8, *P * 4, _lib.BN_TRAIN, 0.1, 1e-5, None, 1, None, 2, 64, 8, 8, _lib.BF16,
                           _lib.NHWC, None) == _lib.EINVAL
    assert lib.mrla_bn_bwd(*P * 5, 8, 0, _lib.BN_TRAIN, 1, None, None, 2, 64, 8, 8, _lib.BF16, _lib.NHWC, None) == _lib.EINVAL
    assert lib.mrla_token_light_fwd(*P * 8, 5, None, None, 1e-6, *P * 4, 2, 17, 64, 16, 1, _lib.F32, None) == _lib.EINVAL
    assert lib.mrla_token_light_bwd(*P * 10, 5, *P * 6, 2, *P * 6, 2, 17, 64, 16, 1, _lib.F32, None) == _lib.EINVAL


def test_model_surface_matches_reference_names():
    from mrla_amd import models
    from oracle import eager_models as em
    names = sorted(n for n in models.__dict__ if n.islower() and not n.startswith("__") and callable(models.__dict__[n]))
    assert "resnet50_mrlal" in names and "resnet101_mrlal" in names
    net = models.resnet50_mrlal(drop_rate=0.0, drop_path=0.2)
    assert set(net.state_dict()) == set(em.eager_resnet50_mrlal().state_dict())
    assert tuple(net.layer1[0].mrla.lambda_t.shape) == (256, 1, 1)
    assert tuple(net.layer4[0].mrla.mrla.Wq.weight.shape) == (1, 1, 7)
    assert net.layer1[0].mrla.mrla.heads == 8 and net.layer1[0].mrla.dim_perhead == 32
    with pytest.raises(ValueError):
        from mrla_amd.layers import mrla_light_layer
        mrla_light_layer(64)


def test_resnet18_mrlal_is_a_labelled_build_side_extension():
    """BASELINE.json's config 1: "resnet18_mrlal forward on 8x3x224x224 random tensors, CPU reference path (plumbing, no GPU)".
    The reference defines no such network; the build's extension (torchvision BasicBlock + the
    reference's light tail) exists under that name, mirrors its eager restatement key for key, and the CPU plumbing runs: the
    eager restatement forwards config 1's input on the host.  (The reference-pinned CPU case stays resnet50_mrlal:
    tests/test_eager_models_golden.py.)"""
    import contextlib
    import io
    from mrla_amd import models, resnet
    from oracle import eager_models as em
    assert "resnet18_mrlal" in models.__all__ and "extension" in (resnet.MRLA_BasicBlock.__doc__ or "").lower()
    with contextlib.redirect_stdout(io.StringIO()):
        net = models.resnet18_mrlal(drop_path=0.1)
    ref = em.eager_resnet18_mrlal()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert [len(getattr(net, f"layer{i}")) for i in (1, 2, 3, 4)] == [2, 2, 2, 2]
    assert tuple(net.layer1[0].mrla.lambda_t.shape) == (64, 1, 1) and net.layer1[0].mrla.mrla.heads == 2
    assert tuple(net.layer1[0].mrla.mrla.Wq.weight.shape) == (1, 1, 3) and tuple(net.layer4[1].mrla.mrla.Wq.weight.shape) == (1, 1, 5)
    assert float(net.layer3[1].bn2.weight.abs().max()) == 0.0                      # zero_init_last_bn reaches the BasicBlock's bn2
    ref.eval()
    with torch.no_grad():
        y = ref(torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(0)))
    assert y.shape == (8, 1000) and torch.isfinite(y).all()
    with pytest.raises(ValueError):
        resnet.MRLA_BasicBlock(64, 64, groups=2)


def test_product_has_no_cpu_fallback():
    from mrla_amd import _lib, models
    net = models.resnet50_mrlal()
    with pytest.raises(_lib.MrlaHipError):
        net(torch.zeros(1, 3, 64, 64))


def test_state_dict_layout_equals_reference():
    """Checkpoint compatibility (resnet/train.py:226-245,333-338): every state_dict key and shape of the reference models,
    recorded from the reference itself in tests/golden/state_dict_layout.json, must be reproduced exactly."""
    import io
    import json
    from contextlib import redirect_stdout

    from mrla_amd import models, vit
    layout = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_layout.json")))
    built = {"resnet50_mrlal": models.resnet50_mrlal, "resnet101_mrlal": models.resnet101_mrlal,
             "resnet50_mrlab": models.resnet50_mrlab, "resnet101_mrlab": models.resnet101_mrlab,
             "deit_mrlal_tiny_patch16_224": vit.deit_mrlal_tiny_patch16_224,
             "deit_mrlal_small_patch16_224": vit.deit_mrlal_small_patch16_224,
             "deit_mrlab_tiny_patch16_224": vit.deit_mrlab_tiny_patch16_224,
             "resnet50_mrlal+SE+ECA": lambda: models.resnet50_mrlal(SE=True, ECA=[3, 5, 5, 7])}
    for name, factory in built.items():
        with redirect_stdout(io.StringIO()):
            sd = factory().state_dict()
        want = layout[name]
        assert set(sd) == set(want), (name, sorted(set(sd) ^ set(want))[:5])
        for k, shape in want.items():
            assert list(sd[k].shape) == shape, (name, k)
    # a checkpoint in the reference's format round-trips through the product model
    with redirect_stdout(io.StringIO()):
        net = models.resnet50_mrlal()
    ckpt = {"epoch": 3, "arch": "resnet50_mrlal", "state_dict": {"module." + k: v.clone() for k, v in net.state_dict().items()}}
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    loaded = torch.load(buf, map_location="cpu")
    with redirect_stdout(io.StringIO()):
        net2 = models.resnet50_mrlal()
    net2.load_state_dict({k[len("module."):]: v for k, v in loaded["state_dict"].items()})   # DDP prefix, as train.py saves it


@pytest.mark.parametrize("layout_name", ["NCHW", "NHWC"])
def test_base_stage_ring_bookkeeping(layout_name):
    """Host logic of the MRLA-base history (mrla_base_module.py:65-70 replaced by rings): the views a layer returns have
    the reference's shapes K[b,t,c], V[b,t,c,h,w] in both storage orders, growth keeps what was written, and the history
    may not grow once its backward pass has begun."""
    from mrla_amd import _lib, functional as Fm
    layout = getattr(_lib, layout_name)
    b, c, h, w, d = 2, 64, 3, 5, 16
    st = Fm.BaseStage(b, c, h, w, d, torch.float32, torch.device("cpu"), 2, layout)
    assert st.T == 2 and st.V.shape == ((2, b, h, w, c) if layout == _lib.NHWC else (b, 2, c, h, w))
    for t in range(5):                                       # capacity hint 2: two doublings on the way to 5 layers
        st.reserve_slot()
        st.slot(st.V, t).fill_(float(t + 1))
        st.K[:, t].fill_(float(-(t + 1)))
        st.t = t + 1
        K, V = st.views()
        assert tuple(K.shape) == (b, t + 1, c) and tuple(V.shape) == (b, t + 1, c, h, w)
        assert K._mrla_stage is st and V._mrla_stage is st
        for j in range(t + 1):
            assert float(V[:, j].min()) == float(V[:, j].max()) == j + 1 and float(K[:, j].max()) == -(j + 1)
    assert st.T == 8
    # one backward pass visits the layers in decreasing order: only its first call reports "new pass" (dK ring re-zeroed)
    assert [st.begin_layer_backward(t) for t in (5, 4, 3, 2, 1)] == [True, False, False, False, False] and st.bwd_top == 5
    # a second pass over the same graph (retain_graph=True) starts at the top again and is recognised as such ...
    assert st.begin_layer_backward(5) is True and st.begin_layer_backward(4) is False
    # ... also when its deepest layer got no gradient this time (bwd_top bounds the dA slots the pass may read)
    assert st.begin_layer_backward(4) is True and st.bwd_top == 4
    assert st.dA.shape == st.V.shape and st.dK.shape == st.K.shape
    st.t = st.T
    with pytest.raises(_lib.MrlaHipError):
        st.reserve_slot()


def test_host_helpers_follow_the_reference_rules():
    """k_size rule (mrla_light_module.py:40-42), heads from dim_perhead (:33-38), stochastic depth (utils/drop.py:7-24)."""
    from mrla_amd import functional as Fm, layers
    from oracle import eager_models as em
    assert [Fm.k_size_for(c) for c in (64, 128, 192, 256, 512, 1024, 2048)] == [3, 5, 5, 5, 5, 5, 7]
    assert all(Fm.k_size_for(c) == em.k_size_for(c) for c in (16, 32, 48, 96, 384, 768, 4096))
    assert layers._heads_and_ksize(256, None, 32, None) == (8, 5) and layers._heads_and_ksize(64, 4, None, 9) == (4, 9)
    assert layers.drop_path_scale(8, 0.0, True, "cpu") is None and layers.drop_path_scale(8, 0.3, False, "cpu") is None
    torch.manual_seed(0)
    s = layers.drop_path_scale(20000, 0.25, True, "cpu")
    assert set(s.unique().tolist()) == {0.0, float(torch.tensor(1.0) / 0.75)}   # dropped, or kept and rescaled
    assert abs(s.mean().item() - 1.0) < 0.02                                    # unbiased in expectation
    # same draw as the reference formula for the same RNG state
    torch.manual_seed(3)
    a = layers.drop_path_scale(64, 0.2, True, "cpu")
    torch.manual_seed(3)
    b = torch.floor(0.8 + torch.rand((64,))) / 0.8
    assert torch.equal(a, b)
    dp = layers.DropPath(0.2).eval()
    x = torch.ones(3, 2, 2)
    assert dp(x) is x


def test_top_level_models_package_serves_train_py_unedited():
    """resnet/train.py:21-26 does `import models` and lists every lowercase callable of models.__dict__ as an --arch choice;
    :158 builds `models.__dict__[arch](drop_rate=..., drop_path=...)`.  With the repository root on PYTHONPATH the
    top-level `models` package makes those lines work as they are."""
    import io
    from contextlib import redirect_stdout

    import models
    names = sorted(n for n in models.__dict__ if n.islower() and not n.startswith("__") and callable(models.__dict__[n]))
    # the reference's four + the two build-side BasicBlock extensions (resnet18 / 34: SURVEY.md section 8(a)-note)
    assert names == ["resnet101_mrlab", "resnet101_mrlal", "resnet18_mrlal", "resnet34_mrlal", "resnet50_mrlab", "resnet50_mrlal"]
    with redirect_stdout(io.StringIO()):
        net = models.__dict__["resnet50_mrlal"](drop_rate=0.0, drop_path=0.2)
    from mrla_amd.resnet import ResNet_mrlal
    assert isinstance(net, ResNet_mrlal) and models.ResNet_mrlal is ResNet_mrlal


def test_parameter_gradient_layout_helper_handles_every_dense_stride_pattern():
    """_grad_like: a row-major gradient buffer handed back with the parameter's own shape and strides (autograd / DDP
    contract; resnet/train.py:174): a view for contiguous and channels_last 1x1 / depthwise weights, a strided copy for any
    other dense layout -- never a silent permutation."""
    import torch
    from mrla_amd.functional import _grad_like
    n, k = 6, 4
    g = torch.arange(n * k, dtype=torch.float32)
    for w in (torch.empty(n, k), torch.empty(n, k, 1, 1), torch.empty(n, k, 1, 1).to(memory_format=torch.channels_last),
              torch.empty(n, 1, 3, 3).to(memory_format=torch.channels_last)):
        gg = torch.arange(w.numel(), dtype=torch.float32)
        out = _grad_like(gg, w.shape, w.stride())
        assert out.shape == w.shape and out.stride() == w.stride()
        assert torch.equal(out.contiguous().view(-1), gg)
        assert out.data_ptr() == gg.data_ptr()                          # a view: no copy kernel on the hot path
    wt = torch.empty(k, n).t()                                          # [n, k] stored column-major: dense, not row-major
    out = _grad_like(g, wt.shape, wt.stride())
    assert out.stride() == wt.stride() and torch.equal(out, g.view(n, k))


def test_bench_py_starts_its_own_ranks_before_touching_the_gpu():
    """`python bench.py --gpus 2` with no torch.distributed environment (resnet/train.py:127-133 spawns its own workers):
    the parent must start `python -m torch.distributed.run ... bench.py <same arguments>` as a child and hand its exit
    code on.  Here there is no GPU, so the two ranks fail at their first device call -- which shows that the launch
    happened, that the parent did not need a GPU to get there, and that it neither prints a line of its own nor reports
    success for failed ranks."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("the CPU form of this test expects the ranks to fail for lack of a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MRLA_DIST_BACKEND"] = "gloo"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--batch", "2", "--no-baselines", "--graph", "0"], env=env, cwd=root, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode(errors="replace")
    assert "torch.distributed.run --nnodes=1 --nproc-per-node=2" in err, err[-2000:]
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
