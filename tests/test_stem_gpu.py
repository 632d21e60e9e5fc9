"""GPU parity of the fused stem tail maxpool3x3/s2/p1(relu(bn1(x))) (mrla_bn_relu_pool_*; resnet_mrla_light.py:220-222)
against the stock modules nn.BatchNorm2d -> relu -> nn.MaxPool2d on the same tensors: outputs, running statistics and every
gradient, train and eval mode, odd / even / ragged spatial sizes, row bands that divide the window rows unevenly, fp32, bf16
and fp16 -- and the sequence route the models take (mrla_stem_fwd / mrla_stem_bwd, no timer) against the per-pass route bit for bit.
(tests/test_stem_exact_gpu.py checks the three kernels exactly, value by value and with guard regions.)"""
import pytest
import torch

from oracle import detgen

pytestmark = pytest.mark.gpu


def _modules(c, seed):
    bn = torch.nn.BatchNorm2d(c).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(1 + 0.3 * detgen.uniform((c,), seed)))
        bn.bias.copy_(torch.from_numpy(0.2 * detgen.uniform((c,), seed + 1)))
    return bn, torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)


# (b, c, h, w): even, odd, ragged last strip (wo % 4 != 0), several bands, two channel groups, tiny
# ... and maps whose window rows the 8 / 32 row bands divide unevenly (Ho = 33, 33, 35, 41, 129), 32 bands with one output column
SHAPES = [(2, 64, 16, 16), (3, 64, 15, 17), (2, 128, 9, 22), (4, 64, 112, 112), (1, 64, 2, 2), (2, 64, 7, 5), (1, 192, 30, 34),
          (1, 64, 66, 4), (1, 64, 65, 8), (1, 64, 70, 4), (1, 64, 82, 4), (1, 64, 258, 32), (1, 64, 256, 2)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_stem_tail_matches_stock_modules(shape, training, dtype):
    from mrla_amd import functional as Fm
    b, c, h, w = shape
    bn, pool = _modules(c, 3)
    bn_r, _ = _modules(c, 3)
    bn.train(training); bn_r.train(training)
    if not training:
        with torch.no_grad():
            for m in (bn, bn_r):
                m.running_mean.copy_(torch.from_numpy(0.1 * detgen.uniform((c,), 7)))
                m.running_var.copy_(torch.from_numpy(1 + 0.2 * detgen.uniform((c,), 8)))
    x0 = torch.from_numpy(detgen.normalish((b, c, h, w), detgen.seed_of(f"stem/{shape}"))).cuda().to(dtype)
    x = x0.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xr = x0.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    Fm.TIMER = timer = Fm.KernelTimer(["mrla_bn_relu_pool_fwd", "mrla_bn_relu_pool_bwd"])
    try:
        out = Fm.bn_relu_maxpool(x, bn, pool)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        assert tuple(out.shape) == (b, c, ho, wo) and out.dtype == dtype
        g = torch.from_numpy(detgen.normalish((b, c, ho, wo), 17)).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
        out.backward(g)
        torch.cuda.synchronize()
    finally:
        Fm.TIMER = None
    assert {n for n, *_ in timer.records} == {"mrla_bn_relu_pool_fwd", "mrla_bn_relu_pool_bwd"}     # the fused path ran
    # stock route on the same values; for bf16 / fp16 through the product's own BatchNorm+ReLU pass (identical rounding), so that
    # the comparison isolates the pooling and its gradient routing
    if dtype == torch.float32:
        a = torch.relu(bn_r(xr))
    else:
        a = Fm.bn_act(xr, bn_r, relu=True)
    out_r = pool(a)
    out_r.backward(g)
    if dtype == torch.float32:
        assert torch.allclose(out, out_r, rtol=1e-5, atol=1e-5)
        tol = 2e-4
    else:
        assert torch.equal(out, out_r)
        tol = 2e-2
    for got, want in ((x.grad, xr.grad), (bn.weight.grad, bn_r.weight.grad), (bn.bias.grad, bn_r.bias.grad)):
        rel = ((got.float() - want.float()).norm() / want.float().norm().clamp_min(1e-20)).item()
        assert rel < tol, rel
    assert torch.allclose(bn.running_mean, bn_r.running_mean, rtol=1e-4, atol=1e-6)
    assert torch.allclose(bn.running_var, bn_r.running_var, rtol=1e-4, atol=1e-6)
    assert int(bn.num_batches_tracked) == int(bn_r.num_batches_tracked)


def _run_stem(shape, training, dtype, timed, x_grad, monkeypatch):
    """One forward + backward of Fm.bn_relu_maxpool on fixed values; per-pass route (a KernelTimer is on) or the sequence
    route.  Returns the C-ABI calls it made, as (entry, arguments), and every result as a CPU tensor."""
    from mrla_amd import _lib as L, functional as Fm
    b, c, h, w = shape
    bn, pool = _modules(c, 3)
    bn.train(training)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(0.1 * detgen.uniform((c,), 7)))
        bn.running_var.copy_(torch.from_numpy(1 + 0.2 * detgen.uniform((c,), 8)))
    x = torch.from_numpy(detgen.normalish(shape, detgen.seed_of(f"stem/{shape}"))).cuda().to(dtype)
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(x_grad)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.from_numpy(detgen.normalish((b, c, ho, wo), 17)).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    calls, call = [], L.call
    with monkeypatch.context() as mp:
        mp.setattr(L, "call", lambda name, *a: (calls.append((name, a)), call(name, *a))[1])
        Fm.TIMER = Fm.KernelTimer(["mrla_bn_relu_pool_fwd", "mrla_bn_relu_pool_bwd"]) if timed else None
        try:
            out = Fm.bn_relu_maxpool(x, bn, pool)
            out.backward(g)
            torch.cuda.synchronize()
        finally:
            Fm.TIMER = None
    res = dict(out=out.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var, batches=bn.num_batches_tracked)
    return calls, {k: None if v is None else v.detach().cpu() for k, v in res.items()}


ROUTE_SHAPES = [(2, 64, 16, 16), (1, 64, 66, 4), (1, 192, 30, 34)]
PER_PASS = {"mrla_bn_relu_pool_fwd", "mrla_bn_relu_pool_dmoments", "mrla_bn_relu_pool_bwd", "mrla_bn_stats_fwd", "mrla_bn_stats_bwd"}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sequence_route_equals_the_per_pass_route_bit_for_bit(shape, training, dtype, monkeypatch):
    """Without a timer the stem is two calls, mrla_stem_fwd and mrla_stem_bwd (what the models run); with one, a call per pass.
    Same kernels on the same buffers: outputs, x.grad, both parameter gradients and the running statistics are bit-identical.
    With a frozen input (x.requires_grad == False) mrla_stem_bwd gets dx == NULL, skips the apply pass and leaves the same
    parameter gradients."""
    per_calls, per = _run_stem(shape, training, dtype, True, True, monkeypatch)
    seq_calls, seq = _run_stem(shape, training, dtype, False, True, monkeypatch)
    fro_calls, fro = _run_stem(shape, training, dtype, False, False, monkeypatch)
    names = lambda calls: [n for n, _ in calls]  # noqa: E731
    assert PER_PASS <= set(names(per_calls)) and not {"mrla_stem_fwd", "mrla_stem_bwd"} & set(names(per_calls))
    for calls in (seq_calls, fro_calls):
        assert {"mrla_stem_fwd", "mrla_stem_bwd"} <= set(names(calls)) and not PER_PASS & set(names(calls))
    dx_arg = lambda calls: [a[8] for n, a in calls if n == "mrla_stem_bwd"]  # noqa: E731
    assert dx_arg(fro_calls) == [None] and len(dx_arg(seq_calls)) == 1 and dx_arg(seq_calls)[0]
    assert fro["dx"] is None and seq["dx"] is not None
    ints = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
    bits = lambda t: t.contiguous().view(ints.get(t.dtype, t.dtype))  # noqa: E731
    for k in per:
        assert seq[k].dtype == per[k].dtype and torch.equal(bits(seq[k]), bits(per[k])), k
        if k != "dx":
            assert torch.equal(bits(fro[k]), bits(seq[k])), k
    assert bool(torch.isfinite(per["dx"].float()).all()) and bool(torch.isfinite(per["out"].float()).all())
    assert float(per["dgamma"].abs().max()) > 0 and float(per["dbeta"].abs().max()) > 0


def test_other_pool_configurations_keep_the_two_step_route():
    from mrla_amd import functional as Fm
    bn, _ = _modules(64, 5)
    x = torch.randn(2, 64, 12, 12, device="cuda").contiguous(memory_format=torch.channels_last)
    for pool in (torch.nn.MaxPool2d(2, 2), torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True), torch.nn.MaxPool2d(3, 1, 1)):
        Fm.TIMER = timer = Fm.KernelTimer(["mrla_bn_relu_pool_fwd"])
        try:
            y = Fm.bn_relu_maxpool(x, bn, pool)
        finally:
            Fm.TIMER = None
        assert not timer.records and torch.allclose(y, pool(torch.relu(bn(x))), atol=1e-5)
    xn = torch.randn(2, 64, 12, 12, device="cuda")                        # NCHW: bn_act + the module's own pooling
    y = Fm.bn_relu_maxpool(xn, bn, torch.nn.MaxPool2d(3, 2, 1))
    assert y.shape == (2, 64, 6, 6)
