"""--dump-outputs DIR: what a step of the timed path computes, as DIR/<name>.npy, so that two builds can be compared output for output.

A training step hands its caller the loss and leaves the gradients and the updated weights behind:
  loss.npy      the loss of the step, float32 [1]
  grads.npy     the gradients of that step, all parameters that have one as one flat vector in module order
  weights.npy   the weights after that step's update, all parameters as one flat vector in module order
The two vectors are written whole up to SAMPLE elements, else as the same SAMPLE positions every time (drawn once from
numpy's default_rng(0) and sorted): 3 x 16 MB at the most.

Which step.  The state the LAST TIMED step starts from is not reproducible: these are real bf16 training steps at lr 0.1 on
random labels, MIOpen accumulates its weight gradients with atomics, and the differences grow from step to step -- after
5 warm-up + 3 capture + 3 check + 20 timed steps two runs of the SAME build on resnet50_mrlal b = 256 differed by 28 % in
the gradients, 10 % in the loss and 1.7 % in the weights (relative L2), which no comparison of two builds can see through.
So, after the timed steps, the single-process run writes back the seeded state it started from (weights as initialised under
torch.manual_seed(0), BatchNorm buffers, zeroed momentum, the generator state: graphs.TrainingState), runs the timed path --
the same replayed graph, or the same eager step -- for STEPS_FROM_SEEDED_STATE steps, untimed, and writes the last of them.
Two steps, not one: the blocks' last BatchNorm weights are initialised to zero, so the first step from that state sends no
gradient into the residual branches; the second one exercises every kernel, and starts from a state that differs between
runs by one step's atomics noise only (measured, two runs of one build: loss identical, weights 2e-10, gradients 2e-7 relative
L2; 4e-5 / 3 % where MIOpen's search had settled on other solvers for the bf16 convolutions).  (With a process group -- N > 1, --ddp-probe -- the state after the timed steps is
written as it is.)  Model, batch and the stochastic-depth masks are seeded, so the same command line gives the same inputs
from run to run."""
import os

import numpy as np
import torch

SAMPLE = 1 << 22
STEPS_FROM_SEEDED_STATE = 2


def _flat_sample(tensors):
    flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
    if flat.numel() > SAMPLE:
        idx = np.sort(np.random.default_rng(0).integers(0, flat.numel(), SAMPLE))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.cpu().numpy().astype(np.float32)


def snapshot(net, loss, grads=None):
    """{name: float32 array} of what the step that just ran left behind.  grads: the gradient tensors it wrote, one entry per
    parameter, where they are not the parameters' .grad (a replayed graph writes the tensors of its capture)."""
    torch.cuda.synchronize()
    params = list(net.parameters())
    out = {"weights": _flat_sample(params)}
    grads = [g for g in (grads if grads is not None else [p.grad for p in params]) if g is not None]
    if grads:
        out["grads"] = _flat_sample(grads)
    if isinstance(loss, torch.Tensor):
        out["loss"] = loss.detach().float().reshape(-1).cpu().numpy().astype(np.float32)
    return out


def write(directory, arrays):
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)
