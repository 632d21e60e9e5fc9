"""The fused MRLA-base token module (mrla_token_base_*: LayerNorm on load, V_t straight into the ring, the flat history kernels
writing the map rows of the token tensor in place) at the widths, map sides and element types the other token tests do not reach.

(a) float32 against the float64 eager module: DeiT-small / DeiT-base widths (384 and 768: 192-thread workgroups of the flat
    kernels, 96 / 192 lanes per pixel), the 1 x 1 map, ragged strips with 4 row bands (side 17, side 24), 9 strips on 8 waves
    (side 57), a five-layer chain that crosses a history reset and grows its rings.
(b) bf16 and fp16, ELEMENTWISE, against oracle.token_base_storage: the same module in float64 with a rounding to the storage
    type at every point where the kernels store one (V_t into the ring, dV_t out of mrla_base_dv_combine, out, dx).  The bound
    on `out` is derived; those on dx and the parameter gradients are 4 x what a float32 run of that same rounding reference
    deviates from its float64 run on the CPU (scripts/token_16bit_bounds.py -> profiles/token_16bit_bounds.md), never anything
    taken from the kernels."""
import functools

import numpy as np
import pytest
import torch

from oracle import detgen, eager_models as em, token_base_storage as ts
from tests import cases
from tests.test_token_base_golden import D, rel

pytestmark = pytest.mark.gpu

FP32_CASES = [(3, 2, 64, 3), (1, 290, 64, 3), (1, 577, 384, 2), (2, 26, 768, 3), (2, 50, 256, 5), (1, 3250, 64, 2)]
STORAGE_CASES = [(2, 17, 64, 4), (2, 50, 128, 3), (2, 197, 192, 3), (1, 290, 64, 3)]
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}          # spacing of the storage type relative to the value, at most


def case_id(case):
    return "b{}n{}c{}x{}".format(*case)


def filled(m, t):
    vals = detgen.fill_state_dict(m.state_dict(), salt=70 + t)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()})
    return m


def product(c, t):
    from mrla_amd import layers
    m = layers.mrlab_module(c, D, init_cell=(t % 4 == 0))
    m.mrla.history_hint = 2           # (the rings grow once inside a stage of more than two layers)
    return filled(m, t)


def inputs(b, n, c, t, storage=None):
    """(x, upstream gradient) of layer t as float32 arrays, rounded to the storage type if one is given."""
    s = detgen.seed_of(f"tokbase-geo/{n}/{c}/{t}")
    x, g = (detgen.normalish((b, n, c), s) * 1.2 + 0.1).astype(np.float32), detgen.normalish((b, n, c), s + 1).astype(np.float32)
    if storage is not None:
        x, g = (torch.from_numpy(a).to(storage).float().numpy() for a in (x, g))
    return x, g


# ------------------------------------------------------------------------------------------------
# (a) float32 (the harness of tests/test_token_base_gpu.py::test_fused_token_module_chain_vs_eager_float64)
# ------------------------------------------------------------------------------------------------
def run(make, case, dev, dtype):
    b, n, c, steps = case
    mods, xs, outs, loss, K, V = [], [], [], 0.0, None, None
    for t in range(steps):
        m = make(c, t).to(dev, dtype)
        x, g = inputs(b, n, c, t)
        x = torch.from_numpy(x).to(dev, dtype).requires_grad_(True)
        y, K, V = m(x, K, V)
        loss = loss + ((x + y) * torch.from_numpy(g).to(dev, dtype)).sum()
        mods.append(m); xs.append(x); outs.append(y)
    loss.backward()
    return mods, xs, outs


@pytest.mark.parametrize("case", FP32_CASES, ids=case_id)
def test_fused_token_module_geometry_fp32_vs_eager_float64(case):
    from mrla_amd import functional as F_
    b, n, c, steps = case
    probe = torch.zeros((b, n, c), device="cuda")
    assert F_.token_base_supported(probe, D), "this case is meant to take the fused path"
    got = run(product, case, "cuda", torch.float32)
    want = run(lambda c_, t: filled(em.EagerTokenBaseModule(c_, D, init_cell=(t % 4 == 0)), t), case, "cpu", torch.float64)
    for t in range(steps):
        assert rel(got[2][t].detach().cpu().numpy(), want[2][t].detach().numpy()) < cases.ACT_TOL, t
        assert rel(got[1][t].grad.cpu().numpy(), want[1][t].grad.numpy()) < cases.ACT_TOL, t
        wp = dict(want[0][t].named_parameters())
        for pn, pv in got[0][t].named_parameters():
            assert rel(pv.grad.cpu().numpy(), wp[pn].grad.numpy()) < (cases.QK_TOL if ("Wq" in pn or "Wk" in pn) else cases.PAR_TOL), (t, pn)


# ------------------------------------------------------------------------------------------------
# (b) 16-bit storage against the rounding reference
# ------------------------------------------------------------------------------------------------
def dx_measure(got, want):
    """The elementwise measure of tests/test_base_gpu.py::assert_mostly_close: the error relative to |want| + 5 % of the
    tensor's maximum; the worst element."""
    want = np.asarray(want, np.float64)
    return (np.abs(np.asarray(got, np.float64) - want) / (np.abs(want) + 0.05 * np.abs(want).max())).max()


def par_measure(got, want):
    """max|got - want| / max|want|, with the floor of test_token_base_golden.rel (dWq / dWk of a layer whose history is its own
    slot alone are exactly zero)."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-9)


def out_excess(got, want, vmax, u):
    """Worst |got - want| over the derived bound of `out`.  The kernels' float32 V_t may round to the neighbouring storage
    value of the reference's float64 V_t (on a small share of elements), a step of at most u * max|V history|; the softmax
    weights are positive and sum to 1, so `out` moves by at most that; its own float32 arithmetic stays within ACT_TOL of the
    maximum (part (a)) and its own rounding adds one spacing of the result:
        |got - want| <= u * |want| + u * max|V history| + ACT_TOL * max|want|."""
    want = np.asarray(want, np.float64)
    tol = u * np.abs(want) + u * vmax + cases.ACT_TOL * np.abs(want).max()
    return (np.abs(np.asarray(got, np.float64) - want) / tol).max()


def reference_chain(case, sname, arith=torch.float64):
    """The rounding reference of a case on the CPU in `arith` arithmetic (float64: the reference; float32: the emulation whose
    distance from it the bounds below are 4 x of)."""
    b, n, c, steps = case
    st = STORAGE[sname]
    return ts.run_chain(lambda t: filled(ts.StorageTokenBaseModule(c, D, init_cell=(t % 4 == 0), storage=st), t),
                        lambda t: inputs(b, n, c, t, st), steps, "cpu", arith, st)


reference = functools.lru_cache(maxsize=None)(reference_chain)

# Worst deviation of the float32 emulation from the float64 reference over STORAGE_CASES and their layers, measured on the CPU
# by scripts/token_16bit_bounds.py (profiles/token_16bit_bounds.md), with dx_measure / par_measure; bound = max(4 x measured,
# one spacing of the storage type).  The factor covers another float32 summation order in the kernels, not another algorithm.
# The emulation has no element beyond its own worst, so no outliers are allowed either.
MEASURED = {
    "bf16": {"dx": 2.818e-03,                  # -> bound 1.127e-02 (1.44 spacings of bf16)
             "normx.weight": 6.705e-05,        # -> bound 2^-7 = 7.812e-03: 4 x measured is below one spacing, here and below
             "normx.bias": 2.274e-05, "mrla.Wq.weight": 2.284e-05, "mrla.Wk.weight": 4.118e-05, "mrla.Wv.weight": 9.681e-05},
    "fp16": {"dx": 4.058e-04,                  # -> bound 1.623e-03 (1.66 spacings of fp16)
             "normx.weight": 1.470e-05,        # -> bound 2^-10 = 9.766e-04, here and below
             "normx.bias": 1.455e-05, "mrla.Wq.weight": 2.992e-05, "mrla.Wk.weight": 1.966e-05, "mrla.Wv.weight": 6.523e-05},
}


def bound(sname, kind):
    return max(4.0 * MEASURED[sname][kind], ULP[sname])


@pytest.mark.parametrize("case", STORAGE_CASES, ids=case_id)
@pytest.mark.parametrize("sname", list(STORAGE))
def test_fused_token_module_16bit_vs_rounding_reference(case, sname):
    from mrla_amd import functional as F_
    b, n, c, steps = case
    st, u = STORAGE[sname], ULP[sname]
    assert F_.token_base_supported(torch.zeros((b, n, c), device="cuda", dtype=st), D), "this case is meant to take the fused path"
    got = ts.run_chain(lambda t: product(c, t), lambda t: inputs(b, n, c, t, st), steps, "cuda", st)
    want = reference(case, sname)
    np_ = lambda a: a.detach().double().cpu().numpy()  # noqa: E731
    worst = {}
    for t in range(steps):
        assert got[2][t].dtype == st and got[1][t].grad.dtype == st
        worst[t, "out"] = out_excess(np_(got[2][t]), np_(want[2][t]), float(want[3][t].abs().max()), u), 1.0
        worst[t, "dx"] = dx_measure(np_(got[1][t].grad), np_(want[1][t].grad)), bound(sname, "dx")
        wp = dict(want[0][t].named_parameters())
        for pn, pv in got[0][t].named_parameters():
            assert pv.grad.dtype == torch.float32
            worst[t, pn] = par_measure(np_(pv.grad), np_(wp[pn].grad)), bound(sname, pn)
    for key, (value, limit) in worst.items():
        print(f"{case_id(case)} {sname} layer {key[0]} {key[1]}: {value:.3e} (bound {limit:.3e})")
    for key, (value, limit) in worst.items():
        assert value <= limit, (key, value, limit)
