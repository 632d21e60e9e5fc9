"""The fp32 model route on the fp32-input MFMA GEMMs (functional.CONV1X1_F32 through fp32_gemms()): a bottleneck with a
strided downsample against the same block with the switch off and a float64 evaluation, resnet50_mrlal in eval and train
mode at the bounds tests/test_models_gpu.py puts on the default route, and a captured training step.

Bounds.  Running statistics: rtol 1e-4, atol 1e-6 against the switch-off block (tests/test_conv1x1_gpu.py's comparison with
the stock modules).  Activations and gradients: the relative L2 error of the switch-OFF block against the float64 CPU
evaluation of the same block is measured in the test (profiles/conv1x1_f32.md records it), and the switch-on block must stay
within twice that error against the same float64 evaluation -- the factor covers a different order of summation; nothing is
compared against the code under test."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import detgen, eager_models as em
from tests import cases
from tests.test_models_gpu import load_det, rel

pytestmark = pytest.mark.gpu
_CL = torch.channels_last


def _downsample(cls=torch.nn.BatchNorm2d):
    return torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, stride=2, bias=False), cls(512))


def _run_block(blk, x0, gup, switch, timer=None):
    from mrla_amd import functional as Fm
    blk = copy.deepcopy(blk)
    x = x0.clone().requires_grad_(True)
    was = Fm.TIMER
    Fm.TIMER = timer
    try:
        with Fm.fp32_gemms(switch):
            out = blk(x)
            out.backward(gup)
    finally:
        Fm.TIMER = was
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"grad:" + k: p.grad for k, p in blk.named_parameters()})
    stats = {k: v.detach().clone() for k, v in blk.state_dict().items() if "running_" in k}
    return res, stats


def _l2(got, want):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    return ((got - want).norm() / want.norm()).item()


REPEATS = 3
TENSORS = ["out", "dx"] + ["grad:" + k for k in (
    "bn1.bias", "bn1.weight", "bn2.bias", "bn2.weight", "bn3.bias", "bn3.weight", "bn_mrla.bias", "bn_mrla.weight",
    "conv1.weight", "conv2.weight", "conv3.weight", "downsample.0.weight", "downsample.1.bias", "downsample.1.weight",
    "mrla.lambda_t", "mrla.mrla.Wk.weight", "mrla.mrla.Wq.weight", "mrla.mrla.Wv.weight")]


def _block_and_inputs():
    from mrla_amd import resnet
    torch.manual_seed(0)
    blk = resnet.MRLA_Bottleneck(256, 128, stride=2, downsample=_downsample()).cuda().to(memory_format=_CL).train()
    load_det(blk)
    x0 = torch.from_numpy(detgen.normalish((2, 256, 14, 14), 11)).float().cuda().contiguous(memory_format=_CL)
    gup = torch.from_numpy(detgen.normalish((2, 512, 7, 7), 12)).float().cuda().contiguous(memory_format=_CL)
    return blk, x0, gup


def _pinned_runs_main(out_path):
    """What the child process of _bottleneck_runs executes: REPEATS runs of the block with the switch off, REPEATS with it
    on, under MIOpen's immediate mode and deterministic solver list; everything to `out_path` as CPU tensors."""
    blk, x0, gup = _block_and_inputs()
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    runs = {switch: [_run_block(blk, x0, gup, switch) for _ in range(REPEATS)] for switch in (False, True)}
    torch.save({switch: [({k: v.cpu() for k, v in r.items()}, {k: v.cpu() for k, v in st.items()}) for r, st in rs]
                for switch, rs in runs.items()}, out_path)


@functools.lru_cache(maxsize=None)
def _bottleneck_runs():
    """The block (input 2 x 256 x 14 x 14, planes 128, stride 2, train mode) with the switch off and on, and the float64 CPU
    evaluation of the eager restatement of the same block -- computed once for every test below.

    The stock convolutions are pinned, so that the switch-off error is a quantity and not a draw:
      * MIOpen's immediate mode and its deterministic solver list -- otherwise the stock forward is not bit-reproducible
        from run to run at these sizes, and the 3-tap gradients of the MRLA gate (sums of nearly cancelling terms) turn
        that last-bit noise into an error that moves by several x on identical inputs;
      * a fresh process with an empty user database (MIOPEN_USER_DB_PATH, as benchkit does for the benchmark): immediate
        mode reads what earlier solver searches of the same user recorded there -- a cudnn.benchmark = True run over these
        shapes changes the backward solvers it picks, to ones that are not reproducible even from the deterministic
        list -- and MIOpen reads that path once per process."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MIOPEN_USER_DB_PATH=os.path.join(tmp, "miopen_db"))
        os.makedirs(env["MIOPEN_USER_DB_PATH"])
        out_path = os.path.join(tmp, "runs.pt")
        subprocess.run([sys.executable, "-m", "tests.test_conv1x1_f32_models_gpu", out_path], cwd=root, env=env, check=True,
                       timeout=240)
        runs = torch.load(out_path)
    (off, stats_off), (on, stats_on) = runs[False][0], runs[True][0]
    blk, x0, gup = _block_and_inputs()
    ref = em.EagerLightBottleneck(256, 128, stride=2, downsample=_downsample()).train()
    ref.load_state_dict({k: v.cpu() for k, v in blk.state_dict().items()})
    ref = ref.double()
    xr = x0.detach().cpu().double().contiguous().requires_grad_(True)
    outr = ref(xr)
    outr.backward(gup.cpu().double().contiguous())
    want = {"out": outr.detach(), "dx": xr.grad}
    want.update({"grad:" + k: p.grad for k, p in ref.named_parameters()})
    _bottleneck_runs.repeats = ([r for r, _ in runs[False]], [r for r, _ in runs[True]])
    return blk, x0, gup, off, on, want, stats_off, stats_on


def test_both_sides_of_the_bottleneck_comparison_are_reproducible():
    """The premise of the 2 x comparison below: with the stock convolutions pinned, REPEATS runs of the switch-off block are
    bit-equal in every tensor, and so are REPEATS runs of the switch-on block -- both errors against float64 are fixed
    quantities of the code, not draws."""
    _, _, _, _, _, want, _, _ = _bottleneck_runs()
    for side, runs in zip(("switch off", "switch on"), _bottleneck_runs.repeats):
        moved = {}
        for k in TENSORS:
            errs = [_l2(r[k], want[k]) for r in runs]
            if not all(torch.equal(r[k], runs[0][k]) for r in runs[1:]):
                moved[k] = errs
        print(f"{side}: {len(moved)} of {len(TENSORS)} tensors differ between {REPEATS} runs", moved)
        assert not moved, (side, moved)


@pytest.mark.parametrize("name", TENSORS)
def test_bottleneck_with_a_strided_downsample_stays_within_twice_the_stock_error(name):
    """Relative L2 error against float64: the switch-on block within 2 x the error of the switch-off block, per tensor,
    with the stock side pinned (_bottleneck_runs) so that both errors are reproducible.  profiles/conv1x1_f32.md section 2
    has the measured figures."""
    _, _, _, off, on, want, _, _ = _bottleneck_runs()
    assert set(want) == set(on) == set(off) == set(TENSORS)
    assert want[name].abs().sum().item() >= 1e-4            # (none of them is a mathematically-zero gradient)
    e_off, e_on = _l2(off[name], want[name]), _l2(on[name], want[name])
    print(f"{name:32s} rel L2 vs float64: switch off {e_off:.3e}  on {e_on:.3e}  ratio {e_on / max(e_off, 1e-300):.2f}")
    assert e_on <= 2 * e_off, (name, e_off, e_on)


def test_bottleneck_running_statistics_and_launches():
    from mrla_amd import functional as Fm
    blk, x0, gup, off, on, want, stats_off, stats_on = _bottleneck_runs()
    assert len(stats_off) == 10
    for k in stats_off:
        assert torch.allclose(stats_on[k], stats_off[k], rtol=1e-4, atol=1e-6), k
    # the new entry points were launched for conv1, conv3 and the downsample, in all three products
    timer = Fm.KernelTimer()
    _run_block(blk, x0, gup, True, timer)
    launches = {k: v["launches"] for k, v in timer.summary().items() if "conv1x1" in k}
    assert launches == {"mrla_conv1x1_f32_fwd": 3, "mrla_conv1x1_f32_bwd_data": 3, "mrla_conv1x1_f32_wgrad": 3}, launches
    timer = Fm.KernelTimer()
    _run_block(blk, x0, gup, False, timer)
    assert not [k for k in timer.summary() if "conv1x1" in k]      # switch off: the stock convolutions, as before


def test_eligible_cases_run_on_the_gemms_or_fall_back_per_operand():
    """Eval mode under no_grad runs on the forward GEMM; a frozen weight gets the input-gradient GEMM and no weight-gradient
    launch; the autograd node alone returns dX and dW in the weight's shape and strides.  Values against float64 at the
    bound of an fp32 chain of fused multiply-adds, (length + 1) 2^-24 sum |a| |b| per element."""
    from mrla_amd import functional as Fm
    k, n = 128, 256
    conv = torch.nn.Conv2d(k, n, 1, bias=False).cuda().to(memory_format=_CL)
    bn = torch.nn.BatchNorm2d(n).cuda()
    x0 = torch.from_numpy(detgen.normalish((2, k, 7, 9), 21)).float().cuda().contiguous(memory_format=_CL)
    m = 2 * 7 * 9

    def rows(t):                                            # [b, c, h, w] -> float64 [m, c]
        return t.detach().double().permute(0, 2, 3, 1).reshape(m, -1)

    w64, x64 = conv.weight.detach().double().reshape(n, k), rows(x0)
    y64 = x64 @ w64.t()
    y_bound = (k + 1) * 2.0 ** -24 * (x64.abs() @ w64.abs().t())

    def run(x, **kw):
        timer = Fm.KernelTimer()
        Fm.TIMER = timer
        try:
            with Fm.fp32_gemms():
                out = Fm.conv_bn_act(x, conv, bn, relu=True, **kw)
        finally:
            Fm.TIMER = None
        return out, timer

    bn.eval()
    with torch.no_grad():
        out, timer = run(x0)
    assert timer.summary()["mrla_conv1x1_f32_fwd"]["launches"] == 1
    sc = 1.0 / (1.0 + bn.eps) ** 0.5                        # fresh running statistics: mean 0, variance 1
    ref = torch.relu(y64 * sc)
    assert ((rows(out) - ref).abs() <= y_bound * sc + 2.0 ** -22 * ref.abs()).all()      # (+ the affine's own roundings)
    bn.train()
    conv.weight.requires_grad_(False)
    x = x0.clone().requires_grad_(True)
    out, timer = run(x)
    Fm.TIMER = timer
    try:
        out.sum().backward()
    finally:
        Fm.TIMER = None
    names = {k_: v["launches"] for k_, v in timer.summary().items() if "conv1x1" in k_}
    assert names == {"mrla_conv1x1_f32_fwd": 1, "mrla_conv1x1_f32_bwd_data": 1}, names
    assert conv.weight.grad is None and x.grad is not None and torch.isfinite(x.grad).all()
    conv.weight.requires_grad_(True)
    # the node alone: y, dX on the weight as stored, dW in the module weight's shape and strides
    g = torch.from_numpy(detgen.normalish((2, n, 7, 9), 22)).float().cuda().contiguous(memory_format=_CL)
    with Fm.fp32_gemms():
        xx = x0.clone().requires_grad_(True)
        y, part = Fm._Conv1x1Fn.apply(xx, conv.weight, False)
    gx, gw = torch.autograd.grad(y, (xx, conv.weight), g)                 # (outside the block: the node remembers its route)
    assert part.numel() == 0 and ((rows(y) - y64).abs() <= y_bound).all()
    g64 = rows(g)
    gx_bound = (n + 1) * 2.0 ** -24 * (g64.abs() @ w64.abs())
    assert ((rows(gx) - g64 @ w64).abs() <= gx_bound).all()
    gw_bound = (m + 1) * 2.0 ** -24 * (g64.abs().t() @ x64.abs())
    assert ((gw.double().reshape(n, k) - g64.t() @ x64).abs() <= gw_bound).all()
    assert gw.shape == conv.weight.shape and gw.stride() == conv.weight.stride() and gw.dtype == torch.float32


def test_resnet50_mrlal_eval_logits_on_the_fp32_gemms():
    from mrla_amd import functional as Fm, models
    torch.backends.cudnn.allow_tf32 = False
    G = cases.golden("models")
    net = models.resnet50_mrlal().cuda()
    ref = em.eager_resnet50_mrlal().cuda()
    load_det(net)
    ref.load_state_dict(net.state_dict())
    net.eval(); ref.eval()
    x = torch.from_numpy(cases.image_batch(8)).cuda()
    timer = Fm.KernelTimer(["mrla_conv1x1_f32_fwd"])
    Fm.TIMER = timer
    try:
        with torch.no_grad(), Fm.fp32_gemms():
            y = net(x)
    finally:
        Fm.TIMER = None
    with torch.no_grad():
        yr = ref(x)
    assert timer.summary()["mrla_conv1x1_f32_fwd"]["launches"] == 36           # 16 x (conv1, conv3) + 4 downsamples
    e_eager, e_golden = rel(y.cpu().numpy(), yr.cpu().numpy()), rel(y.cpu().numpy(), G["resnet50_mrlal/eval8/logits"])
    print(f"eval logits on the fp32 GEMMs: vs eager {e_eager:.3e}, vs golden {e_golden:.3e}")
    assert e_eager < 5e-6                                                      # tests/test_models_gpu.py:35
    assert e_golden < 1e-5                                                     # :36


def test_resnet50_mrlal_train_step_on_the_fp32_gemms():
    from mrla_amd import functional as Fm, models
    G = cases.golden("models")
    net = models.resnet50_mrlal().cuda()
    ref = em.eager_resnet50_mrlal().cuda()
    load_det(net)
    ref.load_state_dict(net.state_dict())
    net.train(); ref.train()
    x = torch.from_numpy(cases.image_batch(4, "img-train")).cuda()
    tgt = (torch.arange(4) * 37 % 1000).cuda()
    with Fm.fp32_gemms():
        y = net(x)
        torch.nn.functional.cross_entropy(y, tgt).backward()
    yr = ref(x)
    torch.nn.functional.cross_entropy(yr, tgt).backward()
    e_eager = rel(y.detach().cpu().numpy(), yr.detach().cpu().numpy())
    e_golden = rel(y.detach().cpu().numpy(), G["resnet50_mrlal/train4/logits"])
    print(f"train logits on the fp32 GEMMs: vs eager {e_eager:.3e}, vs golden {e_golden:.3e}")
    assert e_eager < 2e-5 and e_golden < 2e-5                                  # tests/test_models_gpu.py:51-52
    gp, gr = dict(net.named_parameters()), dict(ref.named_parameters())
    worst, tight, dots = (0.0, ""), (0.0, ""), np.zeros(3)
    for k in gp:
        a, b = gp[k].grad.cpu().numpy().ravel().astype(np.float64), gr[k].grad.cpu().numpy().ravel().astype(np.float64)
        if np.abs(b).sum() < 1e-4:
            continue
        e = np.abs(a - b).sum() / np.abs(b).sum()
        worst = max(worst, (e, k))
        if k.endswith(("mrla.mrla.Wv.weight", "mrla.lambda_t", "bn_mrla.weight", "bn_mrla.bias", "bn3.weight", "bn3.bias")):
            tight = max(tight, (e, k))
        dots += np.array([a @ b, a @ a, b @ b])
    print("model-level gradient check on the fp32 GEMMs: worst", worst, "worst of the MRLA / bn3 parameters", tight)
    assert tight[0] < 2e-2, tight                                              # :70-75
    assert worst[0] < 0.2, worst
    assert dots[0] / np.sqrt(dots[1] * dots[2]) > 0.9999
    sp, sr = net.state_dict(), ref.state_dict()
    for k in ("layer1.0.bn_mrla.running_mean", "layer4.2.bn_mrla.running_var", "layer2.1.bn_mrla.num_batches_tracked"):
        assert rel(sp[k].float().cpu().numpy(), sr[k].float().cpu().numpy()) < 1e-5, k


def test_a_captured_fp32_step_replays_on_the_gemms():
    """mrla_amd.graphed_step on resnet50_mrlal, fp32, batch 8 of 64 x 64 images, with the switch on: its own
    replay-equals-eager verdict is ok, and two replays from the same training state are bit-equal.  MIOpen's deterministic
    solver list is asked for (torch.backends.cudnn.deterministic): the stock 3x3 convolutions otherwise accumulate their
    weight gradients with atomics, run to run in another order (tests/test_graph_replay_gpu.py)."""
    import mrla_amd
    from mrla_amd import models
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        net = models.resnet50_mrlal(drop_path=0.0).cuda().train()
        opt = torch.optim.SGD(net.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(8, 3, 64, 64, device="cuda", generator=g)
        y = torch.randint(0, 1000, (8,), device="cuda", generator=g)
        names = list(net.state_dict())

        def tensors():
            return list(net.state_dict().values()) + [st["momentum_buffer"] for st in opt.state.values()
                                                      if "momentum_buffer" in st]

        def state():
            torch.cuda.synchronize()
            return [v.detach().clone() for v in tensors()]

        def restore(s):
            cur = tensors()
            assert len(cur) == len(s)
            with torch.no_grad():
                for c, v in zip(cur, s):
                    c.copy_(v)

        with mrla_amd.fp32_gemms():
            step = mrla_amd.graphed_step(net, opt, torch.nn.functional.cross_entropy, (x, y), autocast=None)
            assert step.graph is not None and step.report is not None and step.report["ok"], step.report
            step(x, y)                                    # (momentum buffers exist and are non-zero from here on)
            start = state()
            step(x, y)
            first, loss1, out1 = state(), step.loss.detach().clone(), step.output.detach().clone()
            restore(start)
            step(x, y)
            second, loss2, out2 = state(), step.loss.detach().clone(), step.output.detach().clone()
        assert step.last_launch == "graph"
    finally:
        torch.backends.cudnn.deterministic = was
    diff = [names[i] if i < len(names) else f"momentum[{i - len(names)}]" for i, (a, b) in enumerate(zip(first, second))
            if not torch.equal(a, b)]
    print(f"two replays: logits max |diff| {(out1 - out2).abs().max().item():.3g}, loss diff {(loss1 - loss2).abs().item():.3g}, "
          f"{len(diff)} of {len(first)} state tensors differ: {diff[:6]}")
    assert torch.equal(out1, out2) and torch.equal(loss1, loss2)
    assert not diff, f"{len(diff)} of {len(first)} tensors differ between two replays from the same state"


if __name__ == "__main__":            # the child process of _bottleneck_runs
    import sys
    _pinned_runs_main(sys.argv[1])
