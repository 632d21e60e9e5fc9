"""TEST INFRASTRUCTURE ONLY -- the DeiT MRLA-base token module (eager_models.EagerTokenBaseModule, deit/deit_mrla_base.py:204-243)
restated with the roundings of a 16-bit run of the fused HIP token path, forward and backward.

The fused path (functional._TokenBaseFn) computes in float32 and keeps three tensors in the storage type between kernels:
  * V_t = dwconv3x3(LN_x(x) map), written into the stage's ring (mrla_token_base_value_fwd) and read back by every later layer;
  * dV_t, the gradient arriving at V_t from this and all later layers, written by mrla_base_dv_combine;
  * the module's output and dx, each rounded once as it is stored.
dA_t is the map rows of the upstream gradient, which is storage-representable already.  `storage_round` is the straight-through
rounding that restates the first two: the value is rounded on the way forward, and the (accumulated) gradient of the rounded
value on the way back.  The arithmetic type is the caller's: float64 for the reference, float32 for an emulation with the same
rounding points whose distance from the float64 run measures what float32 arithmetic costs (scripts/token_16bit_bounds.py)."""
import torch

from oracle import eager_models as em


class _StorageRound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, storage, round_grad):
        ctx.storage, ctx.round_grad = storage, round_grad
        return v.to(storage).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.round_grad:
            g = g.to(ctx.storage).to(g.dtype)
        return g, None, None


def storage_round(v, storage, round_grad):
    """v rounded to `storage` (to nearest even) in v's own dtype; the gradient passes straight through, rounded if asked."""
    return v if storage is None else _StorageRound.apply(v, storage, round_grad)


class StorageTokenBaseModule(em.EagerTokenBaseModule):
    """EagerTokenBaseModule with V_t / dV_t / out rounded to `storage` (None: no rounding, the parent's arithmetic).  The
    history V it returns holds the rounded values, as the ring does.  dx is the caller's to round (x.grad after backward)."""

    def __init__(self, c, d, init_cell=False, storage=None):
        super().__init__(c, d, init_cell)
        self.storage = storage

    def forward(self, xt, K_prev, V_prev):
        xn = self.normx(xt)
        if self.init_cell:
            K_prev = V_prev = None
        b, n, c = xn.shape
        side = int(round((n - 1) ** 0.5))
        layer = self.mrla
        fmap = xn[:, 1:].reshape(b, side, side, c).permute(0, 3, 1, 2)
        q, k, v = layer.project(fmap)
        v = storage_round(v, self.storage, True)
        if self.init_cell:
            K, V = k.unsqueeze(1), v.unsqueeze(1)
        else:
            K, V = torch.cat([K_prev, k.unsqueeze(1)], 1), torch.cat([V_prev, v.unsqueeze(1)], 1)
        t = K.shape[1]
        logits = torch.einsum("bgd,btgd->bgt", q.view(b, layer.g, layer.d), K.view(b, t, layer.g, layer.d))
        P = torch.softmax(logits * layer.scale, dim=-1)
        out = torch.einsum("bgt,btgn->bgn", P, V.reshape(b, t, layer.g, layer.d * side * side)).reshape(b, c, side * side)
        tokens = torch.cat([xn[:, :1], out.transpose(1, 2)], dim=1)
        return storage_round(tokens, self.storage, False), K, V


def run_chain(make, inputs, steps, dev="cpu", dtype=torch.float64, storage=None):
    """`steps` modules in a row on independent inputs, one backward over the sum of <module output, upstream gradient>.
    make(t) -> module (its parameters keep their own dtype unless `dtype` is a float32 / float64 arithmetic type);
    inputs(t) -> (x, gup) float32 numpy arrays.  Returns (modules, x leaves, outputs, V histories); x.grad holds dx,
    rounded to `storage` where one is given (the kernels store dx in that type)."""
    mods, xs, outs, hist, loss, K, V = [], [], [], [], 0.0, None, None
    acc = dtype if dtype in (torch.float32, torch.float64) else torch.float32
    for t in range(steps):
        m = make(t).to(dev)
        if dtype in (torch.float32, torch.float64):
            m = m.to(dtype)
        x, g = inputs(t)
        x = torch.from_numpy(x).to(dev, dtype).requires_grad_(True)
        y, K, V = m(x, K, V)
        loss = loss + (y.to(acc) * torch.from_numpy(g).to(dev, acc)).sum()
        mods.append(m); xs.append(x); outs.append(y.detach()); hist.append(V.detach())
    loss.backward()
    if storage is not None:
        for x in xs:
            x.grad = x.grad.to(storage).to(x.grad.dtype)
    return mods, xs, outs, hist
