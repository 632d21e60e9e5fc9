"""Run-to-run difference of one FP32 training step's gradients (no autocast) with functional.CONV3X3_WGRAD_F32 off and on: the
run-to-run table of profiles/conv3x3_wgrad_f32.md, by the protocol of scripts/conv3x3_grad_noise.py.
    python scripts/conv3x3_f32_grad_noise.py [batch] [deterministic] [reproducible]
The stock library runs in find mode (torch.backends.cudnn.benchmark) unless `deterministic` is given.  With `reproducible` the
whole run is inside mrla_amd.reproducible_gradients() (the fp32 stem gradient from mrla_stem_conv_f32_wgrad in both settings;
`off` then switches only the 3x3 gradients back to the stock operator): profiles/stem_wgrad_f32.md.  resnet50_mrlal, fp32,
224 x 224, the same weights and data: per setting one warm-up step, then the step is run twice and the two sets of gradients are
compared -- relative L2 over all parameters and over the 3x3 convolution weights, and how many parameters' gradients are
bit-equal.  The last line compares the 3x3 weight gradients of the last `on` step with those of the last `off` step."""
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
torch.manual_seed(0)
with contextlib.redirect_stdout(io.StringIO()):
    net = models.resnet50_mrlal(drop_path=0.0).cuda().to(memory_format=torch.channels_last).train()
with torch.no_grad():              # (the blocks' last BatchNorm starts at weight 0, which makes every 3x3 weight gradient 0)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and not bool(m.weight.any()):
            m.weight.fill_(0.5)
g = torch.Generator(device="cuda").manual_seed(5)
x = torch.randn(batch, 3, 224, 224, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
is3 = sorted(name + ".weight" for name, m in net.named_modules()
             if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.groups == 1)
losses, last = [], {}


reproducible = "reproducible" in sys.argv[2:]


def grads(on):
    net.zero_grad(set_to_none=True)
    with mrla_amd.reproducible_gradients(True) if reproducible else contextlib.nullcontext(), mrla_amd.conv3x3_wgrad_f32(on):
        loss = torch.nn.functional.cross_entropy(net(x), y)
        loss.backward()
    losses.append(float(loss))
    return {k: p.grad.double() for k, p in net.named_parameters()}


def rel(a, b, keys):
    num = sum(float((a[k] - b[k]).pow(2).sum()) for k in keys)
    return (num / sum(float(a[k].pow(2).sum()) for k in keys)) ** 0.5


for on in (False, True, False, True):
    grads(on)                                            # warm-up (find mode), then two runs to compare
    a, b = grads(on), grads(on)
    last[on] = b
    same = sum(torch.equal(a[k], b[k]) for k in a)
    same3 = sum(torch.equal(a[k], b[k]) for k in is3)
    print(f"fp32 batch {batch} switch {'on ' if on else 'off'}: run-to-run relative L2 of the gradients: all parameters "
          f"{rel(a, b, list(a)):.3e}, 3x3 weights {rel(a, b, is3):.3e}; bit-equal {same} of {len(a)} parameters, {same3} of "
          f"{len(is3)} 3x3 weights; losses {'bit-equal' if losses[-1] == losses[-2] else 'differ'}; differing: "
          f"{[k for k in a if not torch.equal(a[k], b[k])][:4]}", flush=True)
print(f"fp32 batch {batch}: 3x3 weight gradients, relative L2 on against off: {rel(last[False], last[True], is3):.3e}")
