"""Scenarios and recorder of the launch-trace golden (tests/golden/launch_trace.json, written by
scripts/record_launch_trace.py; replayed by tests/test_launch_trace_gpu.py).

A trace is what mrla_amd.functional asks of the C ABI for one forward + backward: every `_lib.call` in order, as the entry
name and its arguments classified by `_lib.SIGNATURES` -- integers and floats by value, pointers as NULL (0) / non-NULL (1);
addresses are not part of it -- followed, while a KernelTimer is on, by the timer's (label, nbytes, alg, path) records.
Host-side queries (`*_rows`, `*_supported`, ...) go to the library directly, not through `_lib.call`, and are not in a trace.

Every scenario runs in three modes: "seq" (functional.SEQUENCES on), "perpass" (off) and "timer" (a KernelTimer active).
Each names, per mode, the entry points it exists for: a trace without them is an error at record time and in the test."""
import contextlib
import json

import torch

from tests import cases

MODES = ("seq", "perpass", "timer")
CL = torch.channels_last
BF16 = torch.bfloat16


def _classify(L, name, args):
    sig = L.SIGNATURES[name]
    assert len(sig) == len(args), (name, len(sig), len(args))
    rec = [name]
    for kind, a in zip(sig, args):
        a = getattr(a, "value", a)                      # (a ctypes.c_void_p as well as a plain int)
        if kind is L._P:
            rec.append(0 if not a else 1)
        elif kind is L._F:
            rec.append(float(a))
        else:
            rec.append(int(a))
    return rec


@contextlib.contextmanager
def _mode(mode):
    from mrla_amd import functional as F
    was = F.SEQUENCES, F.TIMER
    F.SEQUENCES, F.TIMER = mode != "perpass", (F.KernelTimer() if mode == "timer" else None)
    try:
        yield F.TIMER
    finally:
        F.SEQUENCES, F.TIMER = was


def missing(scenario, mode, recs):
    """The entry points `scenario` exists for in `mode` that the trace `recs` lacks."""
    names = {r[0] for r in recs}
    return [n for n in scenario.expect[mode] if n not in names]


def trace(scenario, mode, strict=True):
    """The records of one run of `scenario` in `mode`; strict: asserts that the entry points the scenario exists for occur."""
    from mrla_amd import _lib as L
    recs, orig = [], L.call
    L.call = lambda name, *a: (recs.append(_classify(L, name, a)), orig(name, *a))[1]
    try:
        with _mode(mode) as timer:
            scenario.fn()
            torch.cuda.synchronize()
            if timer is not None:
                recs += [["@timer", name, nbytes, alg, path] for name, nbytes, _, _, alg, path in timer.records]
    finally:
        L.call = orig
    lacks = missing(scenario, mode, recs) if strict else None
    assert not lacks, f"{scenario.name}/{mode}: the trace lacks {lacks}; it has {sorted({r[0] for r in recs})}"
    return recs


def first_difference(got, want):
    """None when the traces are equal, else a line naming the first differing record."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"record {i}: got {g}, the golden has {w}"
    if len(got) != len(want):
        return f"{len(got)} records, the golden has {len(want)}; the first {min(len(got), len(want))} agree"
    return None


def pack(traces):
    """{key: records} -> {"table": distinct records, "scenarios": {key: indices into the table}}."""
    table, index, out = [], {}, {}
    for key, recs in traces.items():
        ids = []
        for r in recs:
            k = json.dumps(r)
            if k not in index:
                index[k] = len(table)
                table.append(r)
            ids.append(index[k])
        out[key] = ids
    return {"table": table, "scenarios": out}


def unpack(golden, key):
    return [golden["table"][i] for i in golden["scenarios"][key]]


class Scenario:
    def __init__(self, name, fn, seq, perpass=None, timer=None):
        """seq / perpass / timer: the entry points the trace of that mode must contain (perpass defaults to seq's, timer to
        perpass's)."""
        perpass = seq if perpass is None else perpass
        self.name, self.fn = name, fn
        self.expect = {"seq": seq, "perpass": perpass, "timer": perpass if timer is None else timer}


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _rand(shape, seed, dtype=BF16, cl=True, grad=False):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(shape, device="cuda", generator=gen).to(dtype)
    if cl:
        t = t.contiguous(memory_format=CL)
    return t.requires_grad_(True) if grad else t


def _bn(c, training=True, seed=0):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.6, 1.4)
        bn.bias.uniform_(-0.3, 0.3)
    return bn.train(training)


def _conv(k, n, ksize=1, stride=1, seed=3, dtype=None):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(k, n, ksize, stride=stride, padding=ksize // 2, bias=False).cuda().to(memory_format=CL)
    return conv if dtype is None else conv.to(dtype)


@contextlib.contextmanager
def _flag(name, value):
    from mrla_amd import functional as F
    was = getattr(F, name)
    setattr(F, name, value)
    try:
        yield
    finally:
        setattr(F, name, was)


# ------------------------------------------------------------------------------------------------------
# mrla_light
# ------------------------------------------------------------------------------------------------------
LIGHT_SHAPES = {"nchw": ("s256", 3, 256, 7, 5, 32, torch.float32), "cl": ("s128w", 5, 128, 14, 14, 32, BF16)}


def _light_params(c, mode, salt=21):
    P = cases.block_params(c, salt)
    prm = {k: _dev(v).requires_grad_(True) for k, v in P.items() if "running" not in k}
    rm, rv = _dev(P["bn_mrla.running_mean"]), _dev(P["bn_mrla.running_var"])
    bn = None if mode == "nobn" else dict(weight=prm["bn_mrla.weight"], bias=prm["bn_mrla.bias"], running_mean=rm,
                                          running_var=rv, training=(mode == "train"), momentum=0.1, eps=1e-5)
    return prm, bn


def _light(layout, mode):
    def run():
        from mrla_amd.functional import mrla_light
        name, b, c, h, w, d, dtype = LIGHT_SHAPES[layout]
        fmt = CL if layout == "cl" else torch.contiguous_format
        x, o, gup = cases.light_inputs(name, b, c, h, w)
        xt = _dev(x, dtype).contiguous(memory_format=fmt).requires_grad_(True)
        ot = _dev(o, dtype).contiguous(memory_format=fmt).requires_grad_(True)
        prm, bn = _light_params(c, mode)
        dp = torch.tensor([1.25, 0.0, 1.25, 1.25, 0.0][:b], device="cuda")
        out = mrla_light(xt, prm["mrla.mrla.Wq.weight"], prm["mrla.mrla.Wk.weight"], prm["mrla.mrla.Wv.weight"], d, o_prev=ot,
                         lam=prm["mrla.lambda_t"], bn=bn, dp=dp if bn is not None else None, res=bn is not None)
        out.backward(_dev(gup, dtype).contiguous(memory_format=fmt))
    return run


def _light_deferred(lean):
    """conv3's raw output -> bn_act(defer=True) -> the fused producer of mrla_light (the bottleneck's tail)."""
    def run():
        from mrla_amd import functional as F
        name, b, c, h, w, d, dtype = LIGHT_SHAPES["cl"]
        y3 = _rand((b, c, h, w), 11, grad=True)
        ot = _rand((b, c, h, w), 12, grad=True)
        bn3 = _bn(c, seed=5)
        prm, bn = _light_params(c, "train")
        with _flag("LEAN", lean):
            pre = F.bn_act(y3, bn3, relu=False, defer=True)
            out = F.mrla_light(pre, prm["mrla.mrla.Wq.weight"], prm["mrla.mrla.Wk.weight"], prm["mrla.mrla.Wv.weight"], d,
                               o_prev=ot, lam=prm["mrla.lambda_t"], bn=bn, res=True, pre_activation=True)
            out.backward(_rand((b, c, h, w), 13))
    return run


def _light_infer():
    from mrla_amd import functional as F
    name, b, c, h, w, d, dtype = LIGHT_SHAPES["cl"]
    prm, bn = _light_params(c, "eval")
    with torch.no_grad():
        pre = F.bn_act(_rand((b, c, h, w), 11), _bn(c, False, seed=5), relu=False, defer=True)
        F.mrla_light(pre, prm["mrla.mrla.Wq.weight"], prm["mrla.mrla.Wk.weight"], prm["mrla.mrla.Wv.weight"], d,
                     o_prev=_rand((b, c, h, w), 12), lam=prm["mrla.lambda_t"], bn=bn, res=True, pre_activation=True)


# ------------------------------------------------------------------------------------------------------
# mrla_base
# ------------------------------------------------------------------------------------------------------
def _base_chain(cl, fused, deferred=False):
    """Four MRLA-base layers with their tails on one stage; fused: x is the pre-activation and x_t = relu(x + identity) is
    formed by the pooling pass; deferred (channels_last only): x comes out of bn_act(defer=True)."""
    def run():
        from mrla_amd import functional as F, layers
        b, c, h, w, d, T = 3, 64, 6, 5, 16, 4
        fmt = CL if cl else torch.contiguous_format
        torch.manual_seed(1)
        mods = [layers.mrla_base_module(input_dim=c, init_cell=(t == 0)).cuda() for t in range(T)]
        for m in mods:
            m.mrla.dim_perhead = d
        mods[0].mrla.history_hint = T
        bns = [_bn(c, seed=10 + t) for t in range(T)]
        k = v = None
        loss = 0.0
        for t in range(T):
            xt = _rand((b, c, h, w), 20 + t, cl=False).contiguous(memory_format=fmt).requires_grad_(True)
            idt = _rand((b, c, h, w), 30 + t, cl=False).contiguous(memory_format=fmt).requires_grad_(True) if fused else None
            pre = F.bn_act(xt, _bn(c, seed=40 + t), relu=False, defer=True) if deferred else xt
            y, k, v = layers.base_block_tail(pre, k, v, mods[t], bns[t], torch.nn.Identity(), identity=idt)
            loss = loss + (y.float() * _rand((b, c, h, w), 50 + t, torch.float32, cl=False).contiguous(memory_format=fmt)).sum()
        loss.backward()
    return run


# ------------------------------------------------------------------------------------------------------
# tokens
# ------------------------------------------------------------------------------------------------------
def _token_light():
    from mrla_amd.functional import mrla_token_light
    name, b, n, c, d = cases.TOKEN_CASES[1]
    x, o, gup = cases.token_inputs(name, b, n, c)
    xt, ot = _dev(x).requires_grad_(True), _dev(o).requires_grad_(True)
    prm = {k: _dev(v).requires_grad_(True) for k, v in cases.token_params(c).items()}
    out = mrla_token_light(xt, ot, prm["normx.weight"], prm["normx.bias"], prm["normo.weight"], prm["normo.bias"],
                           prm["mrla.Wq.weight"], prm["mrla.Wk.weight"], prm["mrla.Wv.weight"], prm["lambda_t"], d, res=True)
    out.backward(_dev(gup))


def _token_base():
    from mrla_amd import _lib as L, functional as F
    name, b, n, c, d = cases.TOKEN_CASES[1]
    side = int(round((n - 1) ** 0.5))
    x, _, gup = cases.token_inputs(name, b, n, c)
    prm = {k: _dev(v).requires_grad_(True) for k, v in cases.token_params(c).items()}
    stage = F.BaseStage(b, c, side, side, d, torch.float32, torch.device("cuda", torch.cuda.current_device()), 2, L.NHWC)
    loss = 0.0
    for t in range(2):
        xt = (_dev(x) + 0.1 * t).requires_grad_(True)
        out = F.mrla_token_base(xt, prm["normx.weight"], prm["normx.bias"], prm["mrla.Wq.weight"], prm["mrla.Wk.weight"],
                                prm["mrla.Wv.weight"], d, stage)
        loss = loss + (out * _dev(gup)).sum()
    loss.backward()


# ------------------------------------------------------------------------------------------------------
# BatchNorm nodes
# ------------------------------------------------------------------------------------------------------
def _bn_act(cl, training, defer=False):
    def run():
        from mrla_amd import functional as F
        b, c, h, w = 4, 64, 9, 7
        xt = _rand((b, c, h, w), 60, cl=cl, grad=True)
        y = F.bn_act(xt, _bn(c, training), relu=not defer, defer=defer)
        y.backward(_rand((b, c, h, w), 61, cl=cl))
    return run


def _bn_act_pre_moments():
    from mrla_amd import functional as F
    x, conv, bn = _rand((2, 64, 8, 8), 62, grad=True), _conv(64, 256, dtype=BF16), _bn(256)
    y, part = F._Conv1x1Fn.apply(x, conv.weight, True)
    assert part.numel()
    F.bn_act(y, bn, relu=True, pre_moments=part).backward(_rand((2, 256, 8, 8), 63))


def _bn_relu_maxpool():
    from mrla_amd import functional as F
    x = _rand((2, 64, 16, 16), 64, grad=True)
    y = F.bn_relu_maxpool(x, _bn(64), torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
    y.backward(_rand((2, 64, 8, 8), 65))


def _gate_modules(c, gate):
    from mrla_amd import resnet
    torch.manual_seed(7)
    se = resnet.se_layer(c).cuda() if gate == "se" else None
    eca = resnet.eca_layer(c).cuda() if gate == "eca" else None
    return se, eca


def _bn_gate(gate):
    def run():
        from mrla_amd import functional as F
        b, c, h, w = 2, 64, 7, 7
        se, eca = _gate_modules(c, gate)
        x = _rand((b, c, h, w), 66, grad=True)
        with torch.autocast("cuda", dtype=BF16):        # (as inside the models: the eager gate modules hold fp32 weights)
            out = F.bn_gate(x, _bn(c), se=se, eca=eca)
        out.backward(_rand((b, c, h, w), 67))
    return run


# ------------------------------------------------------------------------------------------------------
# conv_bn_act
# ------------------------------------------------------------------------------------------------------
def _conv_bn(k=64, n=256, hw=8, stride=1, dtype=BF16, relu=True, flags=(), conv_dtype=None, ctx=None, **kw):
    """One forward + backward of conv_bn_act on a [2, k, hw, hw] channels_last input under the module switches `flags`."""
    def run():
        from mrla_amd import functional as F
        conv, bn = _conv(k, n, stride=stride, dtype=conv_dtype), _bn(n)
        x = _rand((2, k, hw, hw), 70, dtype, grad=True)
        ho = (hw + stride - 1) // stride
        with contextlib.ExitStack() as stack:
            for name, value in flags:
                stack.enter_context(_flag(name, value))
            if ctx is not None:
                stack.enter_context(getattr(F, ctx)())
            res = F.conv_bn_act(x, conv, bn, relu=relu, **kw)
            if kw.get("passthrough"):
                out, through = res
                torch.autograd.backward([out, through], [_rand((2, n, ho, ho), 71, dtype), _rand(tuple(through.shape), 72, dtype)])
            else:
                res.backward(_rand((2, n, ho, ho), 71, dtype))
    return run


def _conv_bn_eval_fold():
    from mrla_amd import functional as F
    conv, bn = _conv(64, 256, dtype=BF16), _bn(256, False)
    with torch.no_grad():
        F.conv_bn_act(_rand((2, 64, 8, 8), 70), conv, bn, relu=True)


def _conv_bn_gate():
    from mrla_amd import functional as F
    conv, bn = _conv(64, 256), _bn(256)
    se, eca = _gate_modules(256, "eca")
    x = _rand((2, 64, 8, 8), 70, grad=True)
    with torch.autocast("cuda", dtype=BF16):
        out = F.conv_bn_gate(x, conv, bn, se=se, eca=eca)
    out.backward(_rand((2, 256, 8, 8), 71))


# ------------------------------------------------------------------------------------------------------
# spatial convolutions
# ------------------------------------------------------------------------------------------------------
def _conv3x3(stride, switches, bn=False, node=None):
    """node: the name of the autograd node conv3x3 must answer with ("stock": none of the own ones, conv(x) itself)."""
    def run():
        from mrla_amd import functional as F
        conv = _conv(64, 64, 3, stride)
        x = _rand((2, 64, 16, 16), 80, grad=True)
        with contextlib.ExitStack() as stack, torch.autocast("cuda", dtype=BF16):
            for s in switches:
                stack.enter_context(getattr(F, s)())
            y = F.conv3x3_bn_act(x, conv, _bn(64), relu=True) if bn else F.conv3x3(x, conv)
        got = type(y.grad_fn).__name__
        assert node is None or (not got.startswith("_Conv3x3") if node == "stock" else got == node + "Backward"), (got, node)
        y.backward(_rand(tuple(y.shape), 81))
    return run


def _stem_conv():
    from mrla_amd import functional as F
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=CL)
    x = _rand((2, 3, 32, 32), 82)
    with F.stem_wgrad(), torch.autocast("cuda", dtype=BF16):
        y = F.stem_conv(x, conv)
    y.backward(_rand(tuple(y.shape), 83))


# ------------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------------
def _model(arch):
    def run():
        import io
        from mrla_amd import models
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            net = getattr(models, arch)().cuda().train()
        x = torch.from_numpy(cases.image_batch(8, "img-train")).cuda()
        tgt = (torch.arange(8) * 37 % 1000).cuda()
        with torch.autocast("cuda", dtype=BF16):
            y = net(x)
        torch.nn.functional.cross_entropy(y.float(), tgt).backward()
    return run


_LIGHT_SEQ = ["mrla_light_tail_fwd", "mrla_light_tail_bwd"]
_LIGHT_PP = ["mrla_light_stats_fwd", "mrla_light_gate_fwd", "mrla_light_apply_fwd", "mrla_light_stats_bwd", "mrla_light_bn_bwd",
             "mrla_light_gate_bwd", "mrla_light_apply_bwd", "mrla_reduce_rows2"]
_BN_SEQ = ["mrla_bn_fwd", "mrla_bn_bwd"]
_BN_PP = ["mrla_bn_stats_fwd", "mrla_bn_act_fwd", "mrla_bn_plane_dmoments", "mrla_bn_stats_bwd", "mrla_bn_act_bwd"]
_BASE_CL_PP = ["mrla_base_pool_value_fwd", "mrla_base_gate_fwd", "mrla_base_attend_fwd", "mrla_bn_stats_fwd", "mrla_base_tail_fwd",
               "mrla_base_tail_stats_bwd", "mrla_bn_stats_bwd", "mrla_base_attend_bwd", "mrla_base_pmom_reduce",
               "mrla_base_gate_bwd", "mrla_base_dv_combine", "mrla_base_value_bwd_dv", "mrla_reduce_rows2"]
_BASE_NCHW = ["mrla_base_gate_fwd", "mrla_base_attend_fwd", "mrla_bn_stats_fwd", "mrla_base_tail_fwd", "mrla_base_tail_stats_bwd",
              "mrla_bn_stats_bwd", "mrla_base_attend_bwd", "mrla_base_gate_bwd", "mrla_base_value_bwd", "mrla_reduce_rows2"]
_GEMM = ["mrla_conv1x1_fwd", "mrla_conv1x1_wgrad"]
_FUSED = ["mrla_conv1x1_fwd", "mrla_conv1x1_wgrad_bn"]
_GATE = ["mrla_bn_plane_moments", "mrla_bn_stats_fwd", "mrla_bn_gate_pool", "mrla_bn_gate_fwd", "mrla_bn_gate_sums_bwd",
         "mrla_bn_stats_bwd", "mrla_bn_gate_bwd"]

_ADDEND = {True: "mrla_conv1x1_fwd_addend", False: "mrla_conv1x1_fwd_add"}       # who adds the shortcut's gradient

S = Scenario
SCENARIOS = [
    *[S(f"light_{lay}_{mode}", _light(lay, mode), _LIGHT_SEQ, _LIGHT_PP + (["mrla_light_bn_fwd"] if mode != "nobn" else []))
      for lay in ("nchw", "cl") for mode in ("train", "eval", "nobn")],
    S("light_deferred", _light_deferred(False), _BN_SEQ + _LIGHT_SEQ,
      ["mrla_bn_plane_moments", "mrla_bn_stats_fwd", "mrla_light_stats_fwd_fused", "mrla_light_apply_fwd", "mrla_light_apply_bwd",
       "mrla_bn_stats_bwd", "mrla_bn_act_bwd"]),
    S("light_lean", _light_deferred(True), _BN_SEQ + _LIGHT_SEQ,
      ["mrla_light_stats_fwd_fused", "mrla_light_apply_fwd_fused", "mrla_light_stats_bwd_fused", "mrla_light_apply_bwd_fused",
       "mrla_bn_stats_bwd"]),
    S("light_infer", _light_infer, ["mrla_light_pool_fused", "mrla_light_bn_fwd", "mrla_light_apply_fwd_fused"]),
    S("base_cl", _base_chain(True, False), ["mrla_base_layer_fwd", "mrla_base_layer_bwd"], _BASE_CL_PP),
    S("base_cl_fused", _base_chain(True, True), ["mrla_base_layer_fwd", "mrla_base_layer_bwd"], _BASE_CL_PP),
    S("base_cl_deferred", _base_chain(True, True, True), ["mrla_base_layer_fwd", "mrla_base_layer_bwd"] + _BN_SEQ, _BASE_CL_PP),
    S("base_nchw", _base_chain(False, False), _BASE_NCHW + ["mrla_light_stats_fwd"]),
    S("base_nchw_fused", _base_chain(False, True), _BASE_NCHW + ["mrla_light_stats_fwd_fused"]),
    S("token_light", _token_light, ["mrla_token_light_fwd", "mrla_token_light_bwd"],
      ["mrla_token_norm_pool", "mrla_light_gate_fwd", "mrla_token_apply_fwd", "mrla_token_apply_bwd", "mrla_token_gate_bwd",
       "mrla_token_ln_bwd", "mrla_reduce_rows2"]),
    S("token_base", _token_base, ["mrla_token_base_value_fwd", "mrla_token_base_attend_fwd", "mrla_token_base_attend_bwd",
                                  "mrla_token_base_gate_bwd", "mrla_token_base_value_bwd"]),
    *[S(f"bn_act_{'cl' if cl else 'nchw'}_{'train' if tr else 'eval'}", _bn_act(cl, tr), _BN_SEQ,
        _BN_PP + (["mrla_bn_plane_moments"] if tr else [])) for cl in (False, True) for tr in (True, False)],
    S("bn_act_defer", _bn_act(True, True, defer=True), _BN_SEQ,
      ["mrla_bn_plane_moments", "mrla_bn_stats_fwd", "mrla_bn_plane_dmoments", "mrla_bn_stats_bwd", "mrla_bn_act_bwd"]),
    S("bn_act_pre_moments", _bn_act_pre_moments, _BN_SEQ + _GEMM,
      ["mrla_bn_stats_fwd_rows", "mrla_bn_act_fwd", "mrla_bn_stats_bwd", "mrla_bn_act_bwd"] + _GEMM),
    S("bn_relu_maxpool", _bn_relu_maxpool, ["mrla_stem_fwd", "mrla_stem_bwd"],
      ["mrla_bn_plane_moments", "mrla_bn_stats_fwd", "mrla_bn_relu_pool_fwd", "mrla_bn_relu_pool_dmoments", "mrla_bn_stats_bwd",
       "mrla_bn_relu_pool_bwd"]),
    # (with a KernelTimer on, the BatchNorm + gate node does not apply: bn_act and the eager gate modules)
    S("bn_gate_se", _bn_gate("se"), _GATE, _GATE, _BN_PP),
    S("bn_gate_eca", _bn_gate("eca"), _GATE + ["mrla_eca_gate_fwd", "mrla_eca_gate_bwd"], None, _BN_PP),
    # (with a KernelTimer on, the pair is the two nodes)
    S("conv_bn_fused", _conv_bn(), _FUSED + ["mrla_bn_fwd", "mrla_bn_bwd"], _FUSED + ["mrla_bn_stats_fwd_rows", "mrla_bn_stats_bwd"],
      _GEMM + ["mrla_bn_stats_fwd_rows", "mrla_bn_act_bwd"]),
    S("conv_bn_defer", _conv_bn(relu=False, defer=True), _FUSED, None, _GEMM),
    S("conv_bn_two_nodes", _conv_bn(flags=[("WGRAD_BN", False)]), _GEMM + _BN_SEQ, _GEMM + ["mrla_bn_stats_fwd_rows", "mrla_bn_act_bwd"]),
    S("conv_bn_fuse_dx", _conv_bn(relu=False, fuse_dx=True), ["mrla_conv1x1_fwd", "mrla_conv1x1_wgrad_bn_dx"], None, _GEMM),
    S("conv_bn_fuse_dx_off", _conv_bn(relu=False, fuse_dx=True, flags=[("WGRAD_BN_DX", False)]), _FUSED, None, _GEMM),
    *[S(f"conv_bn_through{'_sub' if sub else ''}{'' if addend else '_noaddend'}",
        _conv_bn(k=256, n=64, hw=16, passthrough=True, subsample=sub, flags=[("SHORTCUT_ADDEND", addend)]),
        _FUSED + [_ADDEND[addend]], None, _GEMM + [_ADDEND[addend]])
      for sub in (None, (2, 2)) for addend in (True, False)],
    S("conv_bn_strided", _conv_bn(k=256, n=512, hw=16, stride=2, relu=False), _FUSED, None, _GEMM),
    S("conv_bn_fp16", _conv_bn(dtype=torch.float16, conv_dtype=torch.float16), _GEMM + _BN_SEQ,
      _GEMM + ["mrla_bn_stats_fwd_rows", "mrla_bn_act_bwd"]),
    S("conv_bn_fp32", _conv_bn(dtype=torch.float32, ctx="fp32_gemms"), ["mrla_conv1x1_f32_fwd", "mrla_conv1x1_f32_wgrad"] + _BN_SEQ,
      ["mrla_conv1x1_f32_fwd", "mrla_conv1x1_f32_wgrad", "mrla_bn_stats_fwd_rows", "mrla_bn_act_bwd"]),
    S("conv_bn_eval_fold", _conv_bn_eval_fold, ["mrla_bn_stats_fwd", "mrla_conv1x1_fwd_affine"]),
    S("conv_bn_gate", _conv_bn_gate, _GEMM + _GATE, None, _GEMM + ["mrla_bn_stats_fwd_rows"]),
    *[S(f"conv3x3_s{s}_wgrad", _conv3x3(s, ["conv3x3_wgrad"], node="_Conv3x3Fn"), ["mrla_conv3x3_wgrad"]) for s in (1, 2)],
    *[S(f"conv3x3_s{s}_fwd", _conv3x3(s, ["conv3x3_fwd"], node="_Conv3x3FwdFn"), ["mrla_conv3x3_fwd"]) for s in (1, 2)],
    S("conv3x3_s1_fwd_dgrad", _conv3x3(1, ["conv3x3_fwd", "conv3x3_dgrad"], node="_Conv3x3FwdFn"), ["mrla_conv3x3_fwd"]),
    S("conv3x3_s2_fwd_dgrad", _conv3x3(2, ["conv3x3_fwd", "conv3x3_dgrad"], node="_Conv3x3FwdFn"),
      ["mrla_conv3x3_fwd", "mrla_conv3x3_dgrad_s2"]),
    # (stride 1 has no input-gradient kernel of its own without the own forward: the scenario holds conv3x3 to conv(x) itself --
    # no own node -- and the trace to no launch)
    S("conv3x3_s1_dgrad", _conv3x3(1, ["conv3x3_dgrad"], node="stock"), []),
    S("conv3x3_s2_dgrad", _conv3x3(2, ["conv3x3_dgrad"], node="_Conv3x3Fn"), ["mrla_conv3x3_dgrad_s2"]),
    S("conv3x3_bn_act_fwd", _conv3x3(1, ["conv3x3_fwd"], bn=True), ["mrla_conv3x3_fwd", "mrla_bn_fwd"],
      ["mrla_conv3x3_fwd", "mrla_bn_stats_fwd_rows"]),
    S("stem_conv", _stem_conv, ["mrla_stem_conv_wgrad"]),
    S("resnet50_mrlal", _model("resnet50_mrlal"),
      ["mrla_weight_bank_refresh_dt", "mrla_stem_fwd", "mrla_light_tail_fwd", "mrla_light_tail_bwd", "mrla_conv1x1_wgrad_bn",
       "mrla_conv1x1_wgrad_bn_dx", "mrla_conv1x1_fwd_addend", "mrla_bn_bwd", "mrla_stem_bwd"],
      ["mrla_weight_bank_refresh_dt", "mrla_bn_relu_pool_fwd", "mrla_light_stats_fwd_fused", "mrla_light_apply_bwd",
       "mrla_conv1x1_wgrad_bn", "mrla_conv1x1_wgrad_bn_dx", "mrla_bn_stats_bwd"],
      ["mrla_weight_bank_refresh_dt", "mrla_bn_relu_pool_fwd", "mrla_light_stats_fwd_fused", "mrla_light_apply_bwd",
       "mrla_conv1x1_wgrad", "mrla_bn_stats_fwd_rows", "mrla_bn_act_bwd"]),
    S("resnet50_mrlab", _model("resnet50_mrlab"),
      ["mrla_weight_bank_refresh_dt", "mrla_base_layer_fwd", "mrla_base_layer_bwd", "mrla_conv1x1_wgrad_bn"],
      ["mrla_weight_bank_refresh_dt", "mrla_base_pool_value_fwd", "mrla_base_value_bwd_dv", "mrla_conv1x1_wgrad_bn"],
      ["mrla_weight_bank_refresh_dt", "mrla_base_pool_value_fwd", "mrla_base_value_bwd_dv", "mrla_conv1x1_wgrad"]),
]
BY_NAME = {s.name: s for s in SCENARIOS}
assert len(BY_NAME) == len(SCENARIOS)
