"""GPU: the three 3x3 call sites of mrla_amd/resnet.py (the bottleneck's conv2, both convolutions of the basic block) under
DEFAULT switches at a shape mrla_conv3x3_wgrad_preferred answers 1 for -- 512 -> 512 on 7 x 7 maps at batch 64, the last stage of
a batch-64 step.  No switch context is entered on the routed side.

functional._own_wgrad is wrapped (the product code is not changed): the wrapper records clones of the dy and x it received and
of the gradient it returned.  Per block: the number of launches (one, two), every recorded gradient inside the fp32 summation
bound of tests/test_conv3x3_wgrad_gpu.py against the float64 gradient of the recorded x and dy, the module's .grad bit-equal to
what the wrapper saw returned; and against the same step under conv3x3_wgrad_auto(False), both under cudnn.deterministic: the
loss within 2 bf16 ulps, every parameter gradient within the 2 % relative L2 of tests/test_block_bf16_gpu.py."""
import contextlib

import pytest
import torch

from tests.test_conv3x3_wgrad_auto_gpu import CL, _bits, _defaults, _deterministic, _dw64_taps

pytestmark = pytest.mark.gpu
BATCH, MAP = 64, 7
BLOCKS = {                       # name -> (constructor arguments, input channels, the 3x3 convolutions in backward order)
    "bottleneck": ((2048, 512), 2048, ("conv2",)),
    "basic": ((512, 512), 512, ("conv2", "conv1")),
}


def _build(name):
    from mrla_amd import resnet
    args, cin, convs = BLOCKS[name]
    torch.manual_seed(0)
    blk = (resnet.MRLA_Bottleneck if name == "bottleneck" else resnet.MRLA_BasicBlock)(*args)
    blk = blk.cuda().to(memory_format=CL).train()
    with torch.no_grad():          # a last BatchNorm that starts at weight 0 would make every 3x3 weight gradient exactly 0
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
                m.weight.fill_(0.5)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.relu(torch.randn((BATCH, cin, MAP, MAP), device="cuda", generator=g) + 0.3).bfloat16().contiguous(memory_format=CL)
    proj = torch.rand((BATCH, args[1] * blk.expansion, MAP, MAP), device="cuda", generator=g).contiguous(memory_format=CL)
    return blk, x, proj


def _step(name, ctx):
    """One forward and backward from the fixed seed: (loss, {parameter name: gradient}, the block)."""
    blk, x, proj = _build(name)
    x.requires_grad_(True)
    with ctx, torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
        loss = (out.float() * proj).sum() / BATCH            # a fixed random projection of the output
        loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {k: p.grad for k, p in blk.named_parameters()}, blk


def test_the_block_shapes_are_preferred_ones():
    from mrla_amd import _lib as L
    from mrla_amd import resnet
    _defaults()
    for dt in (L.BF16, L.F16):
        assert L.load().mrla_conv3x3_wgrad_preferred(BATCH, 512, 512, MAP, MAP, 1, dt) == 1
    assert L.conv3x3_wgrad_plan(BATCH, 512, 512, MAP, MAP, 1, L.BF16)[2] * MAP >= 384
    for name, (args, cin, convs) in BLOCKS.items():
        blk = (resnet.MRLA_Bottleneck if name == "bottleneck" else resnet.MRLA_BasicBlock)(*args)
        for conv in convs:
            m = getattr(blk, conv)
            assert (m.in_channels, m.out_channels, m.kernel_size, m.stride, m.bias) == (512, 512, (3, 3), (1, 1), None)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_a_block_step_under_default_switches_takes_its_3x3_weight_gradients_from_the_own_kernel(name, monkeypatch):
    import mrla_amd
    Fm = _defaults()
    convs = BLOCKS[name][2]
    seen, inner = [], Fm._own_wgrad

    def recording(ctx, entry, rows_entry, dy, x, shape, taps):
        gw = inner(ctx, entry, rows_entry, dy, x, shape, taps)
        seen.append((entry, tuple(shape), dy.clone(), x.clone(), None if gw is None else gw.clone()))
        return gw
    monkeypatch.setattr(Fm, "_own_wgrad", recording)

    with _deterministic():
        loss0, g0, _ = _step(name, mrla_amd.conv3x3_wgrad_auto(False))
        assert len(seen) == 0
        loss1, g1, blk = _step(name, contextlib.nullcontext())
    assert len(seen) == len(convs)
    m = BATCH * MAP * MAP
    for (entry, shape, dy, x, gw), conv in zip(seen, convs):
        assert entry == "mrla_conv3x3_wgrad" and shape == (BATCH, 512, 512, MAP, MAP, 1)
        assert dy.dtype == x.dtype == torch.bfloat16 and gw is not None and gw.dtype == torch.float32
        x64, dy64 = x.double().cpu(), dy.double().cpu()
        want64, a = (t.permute(0, 3, 1, 2) for t in (_dw64_taps(x64, dy64, 1), _dw64_taps(x64.abs(), dy64.abs(), 1)))
        assert float(want64.abs().max()) > 0
        err = (gw.double().cpu() - want64).abs()
        print(f"{name}.{conv}: max |dw - dw64| / A = {float((err / a.clamp_min(1e-300)).max()):.3e} "
              f"(the bound {(m + 9) * 2.0 ** -24:.3e})")
        assert bool((err <= (m + 9) * 2.0 ** -24 * a).all()), float((err / a.clamp_min(1e-300)).max())
        weight = getattr(blk, conv).weight
        assert weight.grad.dtype == torch.float32 and weight.grad.stride() == weight.stride()
        assert torch.equal(_bits(weight.grad), _bits(gw)), conv          # the module's gradient is that tensor
    if len(seen) == 2:
        assert not torch.equal(seen[0][4], seen[1][4])

    print(name, f"losses: unrouted {loss0!r} routed {loss1!r}")
    ulp = 2.0 ** (torch.tensor(abs(loss0)).log2().floor().item() - 7)
    assert abs(loss1 - loss0) <= 2 * ulp, (loss0, loss1)
    errs = {}
    assert set(g0) == set(g1)
    for key, a in g0.items():
        assert (a is None) == (g1[key] is None), key
        if a is None:
            continue
        a, b = a.double(), g1[key].double()
        assert bool(torch.isfinite(b).all()), key
        if float(a.norm()) == 0:                             # (a gradient that is exactly 0 on one side is so on the other)
            assert float(b.norm()) == 0, key
            continue
        errs[key] = float((b - a).norm() / a.norm())
    print(name, "parameter gradients, relative L2 routed against unrouted:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert {c + ".weight" for c in convs} <= set(errs)
    for key, e in errs.items():                              # the 3x3 weights and every other parameter: the same 2 %
        assert e < 2e-2, f"grad {key}: relative L2 difference {e:.3e}"
