"""Run-to-run difference of one training step's gradients with functional.CONV3X3_WGRAD off and on: the "parent differs from
itself" figure of profiles/conv3x3_wgrad.md.
    python scripts/conv3x3_grad_noise.py [batch] [stem] [fwd] [dgrad] [deterministic]
With `stem` the `on` runs turn functional.STEM_WGRAD on as well (mrla_amd.reproducible_gradients()): the table of
profiles/stem_wgrad.md; with `fwd` they turn on functional.CONV3X3_FWD on top of both: the table of
profiles/conv3x3_fwd.md; with `dgrad` functional.CONV3X3_DGRAD on top of those three (every own switch): the table of
profiles/conv3x3_dgrad.md.  With `deterministic` the stock library runs its deterministic solvers
(torch.backends.cudnn.deterministic, no find mode): what is left then is the gradient kernels' own run-to-run difference,
without a forward pass that differs from run to run in front of them.  The line also says whether the two losses are bit-equal.
resnet50_mrlal, bf16 autocast, 224 x 224, the same weights and data: the step is run twice per setting and the two sets of
gradients are compared -- relative L2 over all parameters and over the 3x3 convolution weights, and how many parameters'
gradients are bit-equal."""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mrla_amd  # noqa: E402
from mrla_amd import models  # noqa: E402

torch.backends.cudnn.benchmark = "deterministic" not in sys.argv[2:]
torch.backends.cudnn.deterministic = "deterministic" in sys.argv[2:]
batch = int(sys.argv[1]) if len(sys.argv) > 1 else 64
switch = mrla_amd.reproducible_gradients if "stem" in sys.argv[2:] else mrla_amd.conv3x3_wgrad
if "fwd" in sys.argv[2:] or "dgrad" in sys.argv[2:]:
    @contextlib.contextmanager
    def switch(on):
        with mrla_amd.conv3x3_fwd(on), mrla_amd.reproducible_gradients(on), mrla_amd.conv3x3_dgrad(on and "dgrad" in sys.argv[2:]):
            yield
torch.manual_seed(0)
with contextlib.redirect_stdout(io.StringIO()):
    net = models.resnet50_mrlal(drop_path=0.0).cuda().train()
with torch.no_grad():              # (the blocks' last BatchNorm starts at weight 0, which makes every 3x3 weight gradient 0)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
            m.weight.fill_(0.5)
g = torch.Generator(device="cuda").manual_seed(5)
x = torch.randn(batch, 3, 224, 224, device="cuda", generator=g)
y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
is3 = {name + ".weight" for name, m in net.named_modules()
       if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1}


losses = []


def grads(on):
    net.zero_grad(set_to_none=True)
    with switch(on), torch.autocast("cuda", dtype=torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(net(x), y)
        loss.backward()
    losses.append(float(loss))
    return {k: p.grad.double() for k, p in net.named_parameters()}


for on in (False, True, False, True):
    grads(on)                                            # warm-up (find mode), then two runs to compare
    a, b = grads(on), grads(on)
    def rel(keys):
        num = sum(float((a[k] - b[k]).pow(2).sum()) for k in keys)
        return (num / sum(float(a[k].pow(2).sum()) for k in keys)) ** 0.5
    same = sum(torch.equal(a[k], b[k]) for k in a)
    same3 = sum(torch.equal(a[k], b[k]) for k in is3)
    print(f"batch {batch} {'all four switches' if 'dgrad' in sys.argv[2:] else 'all three switches' if 'fwd' in sys.argv[2:] else 'both switches' if switch is mrla_amd.reproducible_gradients else 'switch'} {'on ' if on else 'off'}: run-to-run relative L2 of the gradients: all parameters {rel(list(a)):.3e}, "
          f"3x3 weights {rel(sorted(is3)):.3e}; bit-equal {same} of {len(a)} parameters, {same3} of {len(is3)} 3x3 weights"
          f"; losses {'bit-equal' if losses[-1] == losses[-2] else 'differ'}; differing: {[k for k in a if not torch.equal(a[k], b[k])][:4]}",
          flush=True)
