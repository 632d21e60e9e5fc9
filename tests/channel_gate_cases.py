"""Deterministic inputs, parameters and the float64 restatement of gate(BatchNorm2d(y)) shared by the channel-attention
tests and scripts/make_channel_gate_golden.py (which writes tests/golden/channel_gate.npz from the reference's own modules).

The restatement is the train-mode BatchNorm used elsewhere in the suite (biased variance for normalisation, unbiased for the
running update) followed by the gate (modules/eca_module.py:24-34, modules/se_module.py:19-23), differentiated by torch
autograd in double."""
import numpy as np

from oracle import detgen

EPS, MOMENTUM = 1e-5, 0.1

# golden cases: (name, b, c, h, w, gate) -- gate "eca<k>" or "se"
GOLDEN_CASES = [("eca3_64", 2, 64, 7, 7, "eca3"), ("se_64", 2, 64, 7, 7, "se"), ("eca5_256", 2, 256, 7, 5, "eca5")]
F64_STRIDE = 16                # float64 out / dx are stored as every 16th element of the NCHW-flat tensor
BIG_STRIDE = 16                # so are the float32 ones, and the inputs, of cases above FULL_LIMIT elements;
SMALL_STRIDE = 2               # up to FULL_LIMIT elements: the inputs in full, float32 out / dx as every 2nd element
FULL_LIMIT = 8192              # (the fixture stays under 200 KB)


def inputs(b, c, h, w, tag="gate"):
    """(y, do): the convolution output in front of the BatchNorm (channel means and spreads that differ) and the gradient
    arriving at the node's output, float32 NCHW."""
    s = detgen.seed_of(f"{tag}/{b}x{c}x{h}x{w}")
    mu = detgen.normalish((1, c, 1, 1), s + 1) * 0.5
    sd = 0.5 + detgen.uniform((1, c, 1, 1), s + 2, 0.0, 1.0)
    y = (detgen.normalish((b, c, h, w), s) * sd + mu).astype(np.float32)
    do = detgen.normalish((b, c, h, w), s + 3).astype(np.float32)
    return y, do


def params(c, gate, salt=0):
    """BatchNorm parameters / running statistics and the gate's weights under the reference's key names."""
    s = detgen.seed_of(f"gate-params/{c}/{gate}", salt)
    p = {"bn.weight": (1.0 + 0.3 * detgen.normalish((c,), s)).astype(np.float32),
         "bn.bias": (0.2 * detgen.normalish((c,), s + 1)).astype(np.float32),
         "bn.running_mean": (0.3 * detgen.normalish((c,), s + 2)).astype(np.float32),
         "bn.running_var": (0.5 + detgen.uniform((c,), s + 3, 0.0, 1.0)).astype(np.float32)}
    if gate == "se":
        r = c // 16
        p["se.fc.0.weight"] = (detgen.normalish((r, c), s + 4) * (2.0 / np.sqrt(c))).astype(np.float32)
        p["se.fc.2.weight"] = (detgen.normalish((c, r), s + 5) * (2.0 / np.sqrt(r))).astype(np.float32)
    else:
        k = int(gate[3:])
        p["eca.conv.weight"] = (detgen.normalish((1, 1, k), s + 4) * 0.8).astype(np.float32)
    return p


def gate_keys(gate):
    return ["se.fc.0.weight", "se.fc.2.weight"] if gate == "se" else ["eca.conv.weight"]


def restate_f64(y, do, p, gate, training):
    """out, dy, every parameter gradient and the updated running statistics of gate(BatchNorm2d(y)) in float64.
    `y`, `do`, `p`: numpy arrays (the values are taken as they are: round them to the storage type first where wanted)."""
    import torch
    import torch.nn.functional as F
    t = lambda a, g=True: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=g)      # noqa: E731
    yt, gamma, beta = t(y), t(p["bn.weight"]), t(p["bn.bias"])
    rm, rv = t(p["bn.running_mean"], False), t(p["bn.running_var"], False)
    b, c, h, w = yt.shape
    n = b * h * w
    if training:
        mean = yt.mean((0, 2, 3))
        var = ((yt - mean.view(1, c, 1, 1)) ** 2).mean((0, 2, 3))
        new_rm = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
        new_rv = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * (n / max(n - 1, 1))
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    z = (yt - mean.view(1, c, 1, 1)) / torch.sqrt(var.view(1, c, 1, 1) + EPS) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    pooled = z.mean((2, 3))
    ws = [t(p[k]) for k in gate_keys(gate)]
    if gate == "se":
        a = torch.relu(pooled @ ws[0].t()) @ ws[1].t()
    else:
        k = ws[0].shape[-1]
        a = F.conv1d(pooled.unsqueeze(1), ws[0], padding=(k - 1) // 2).squeeze(1)
    out = z * torch.sigmoid(a).view(b, c, 1, 1)
    (out * t(do, False)).sum().backward()
    res = {"out": out.detach().numpy(), "dx": yt.grad.numpy(), "grad/bn.weight": gamma.grad.numpy(),
           "grad/bn.bias": beta.grad.numpy(), "new_rm": new_rm.numpy(), "new_rv": new_rv.numpy()}
    for k, wt in zip(gate_keys(gate), ws):
        res["grad/" + k] = wt.grad.numpy()
    return res


def sample(a, stride):
    return np.ascontiguousarray(np.asarray(a).reshape(-1)[::stride])


def strides_of(numel):
    """(stride of the stored inputs, stride of the stored float32 out / dx) of a golden case with `numel` elements."""
    return (1, SMALL_STRIDE) if numel <= FULL_LIMIT else (BIG_STRIDE, BIG_STRIDE)


def input_key(b, c, h, w):
    """Cases of one shape share their inputs: stored once, under the shape."""
    return f"in/{b}x{c}x{h}x{w}"


class recorded:
    """Every C-ABI entry the library is asked for inside the block, as (name, args), in order (functional._call and
    the sequence entry points both go through _lib.call)."""

    def __enter__(self):
        from mrla_amd import _lib as L
        self.calls, self._call = [], L.call
        L.call = lambda name, *a: (self.calls.append((name, a)), self._call(name, *a))[1]
        return self.calls

    def __exit__(self, *exc):
        from mrla_amd import _lib as L
        L.call = self._call
