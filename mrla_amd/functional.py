"""torch.autograd wrappers around the C ABI (include/mrla_hip.h).

PyTorch is plumbing here: it owns the device buffers and the stream and records the autograd edge; all
arithmetic of the MRLA path happens in libmrla_hip.so.  There is deliberately no fallback: CPU tensors or
a missing library raise.
"""
import contextlib
import ctypes
import functools
import threading
import weakref
from math import log

import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def k_size_for(c):
    """Conv1d tap count of Wq / Wk (reference: mrla_light_module.py:40-42)."""
    t = int(abs((log(c, 2) + 1) / 2.0))
    return t if t % 2 else t + 1


class KernelTimer:
    """Optional HIP-event timing of selected C-ABI launches on the stream they are launched on (used by
    bench.py for the roofline figure).  Events are read back only after the caller synchronises."""

    def __init__(self, names=None):
        self.names = None if names is None else set(names)       # None: every C-ABI launch
        self.records = []          # (name, nbytes, start_event, end_event, alg_bytes, path_bytes)

    def summary(self):
        """Per label: launches, ms, `bytes` (what the launch is built to move), `bytes_alg` (SURVEY.md section 8(d)'s
        algorithmic count for that launch where it differs) and `bytes_path` (its share of the section-8(d) compulsory bytes
        of the whole MRLA block, attributed to the pass that completes a direction; 0 for the other passes)."""
        out = {}
        for name, nbytes, e0, e1, alg, path in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, bytes=0, bytes_alg=0, bytes_path=0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["bytes"] += nbytes
            d["bytes_alg"] += nbytes if alg is None else alg
            d["bytes_path"] += path
        return out


TIMER = None      # set to a KernelTimer to time launches
SEQUENCES = True  # a tail / BatchNorm direction = ONE call of a sequence entry point (mrla_light_tail_fwd, mrla_bn_bwd, ...;
#                   include/mrla_hip.h ABI 4) instead of one call per pass.  Same kernels, same buffers, bit-identical
#                   results; per-pass calls are used while a KernelTimer is on (events around every kernel) or when False.


LEAN = False      # True: the fused training tail does not store x_t where the library can re-form it (mrla_light_lean_supported:
#                   13N instead of 15N elements of HBM traffic per block and step, 1N less activation memory, bit-identical
#                   results).  Not the default: inside the resnet50_mrlal step the two forms take the same time on MI355X
#                   (29.96 - 29.99 ms lean, 29.80 - 29.95 ms stored: the backward statistics pass pays for re-forming x_t
#                   what the forward one saves, profiles/r06_notes.md section 3) -- switch it on for the memory.


SHORTCUT_ADDEND = True   # conv1's input-gradient GEMM takes the block's shortcut gradient as its addend in every kernel form
#                          and straight from the compact gradient of a strided downsample (mrla_conv1x1_fwd_addend).  False:
#                          only the wide form adds a full-size one (mrla_conv1x1_fwd_add); a torch add, and a zero-fill +
#                          scatter for the strided blocks, do the rest -- the same values, kept for A/B runs and tests.


WGRAD_BN = True   # a 1x1 GEMM convolution + BatchNorm2d pair is one autograd node whose backward forms the BatchNorm's input
#                   gradient inside the weight-gradient GEMM (mrla_conv1x1_wgrad_bn) instead of in an apply pass of its own.
#                   False: the two nodes and the per-pass route -- the same values bit for bit, kept for A/B runs and tests.


CONV1X1_F32 = False   # an fp32 channels_last 1x1 convolution outside autocast (the recipe of resnet/train.py:397-409) runs on the
#                        fp32-input MFMA GEMMs (mrla_conv1x1_f32_fwd / _wgrad): forward with the BatchNorm moment records, input
#                        gradient on the weight as stored, weight gradient -- the strided downsamples included.  False (the
#                        default): fp32 convolutions stay on the stock kernels, launch for launch as before; fp32_gemms() turns it
#                        on for a block of code.  profiles/conv1x1_f32.md has the numbers a change of the default rests on.


def _switch(flag, name):
    """The context manager `name` of the module-level switch `flag`."""
    @contextlib.contextmanager
    def manager(enabled=True):
        g = globals()
        prev, g[flag] = g[flag], bool(enabled)
        try:
            yield
        finally:
            g[flag] = prev
    manager.__name__ = manager.__qualname__ = name
    manager.__doc__ = f"{flag} = `enabled` inside the block; the previous value comes back on exit, also when the block raises."
    return manager


fp32_gemms = _switch("CONV1X1_F32", "fp32_gemms")


CONV3X3_WGRAD = False   # the weight gradient of an eligible 3x3 convolution (conv3x3_applies: the bottleneck's conv2, both of the
#                         basic block's) comes from mrla_conv3x3_wgrad -- fixed split, fixed summation order, no atomics:
#                         bit-reproducible, and right under graph replay at the small batches where the stock library's
#                         split-K solver is not -- written straight as the fp32 master weight's gradient.  Forward and input
#                         gradient stay the stock operator's.  False (the default): conv(x) itself, the very same autograd
#                         graph and launches as before; conv3x3_wgrad() turns it on for a block of code: EVERYWHERE the
#                         kernel applies, also where it is the slower one (stride 2, small batches).
#                         profiles/conv3x3_wgrad.md has the numbers.


conv3x3_wgrad = _switch("CONV3X3_WGRAD", "conv3x3_wgrad")


CONV3X3_WGRAD_AUTO = True   # the same route by shape: an eligible 3x3 convolution takes its weight gradient from
#                             mrla_conv3x3_wgrad where the library expects it to take less device time than everything the
#                             stock operator launches for that gradient (mrla_conv3x3_wgrad_preferred: a rule in the planner's
#                             quantities, derived in profiles/conv3x3_wgrad.md section 7 -- the stride-1 convolutions of a
#                             large-batch step; no stride-2 one, nothing at batch 8 / 16).  What changes numerically at a
#                             routed shape: the gradient is bit-reproducible, and an fp32 master weight receives the fp32 sums
#                             where the stock path hands back a bf16-rounded gradient (1.7e-3 relative L2 apart:
#                             tests/test_conv3x3_route_gpu.py).  Everything else -- and every shape with this switch and
#                             CONV3X3_WGRAD off -- is conv(x) itself, the same autograd graph and launches as before;
#                             conv3x3_wgrad_auto(False) turns it off for a block of code.


conv3x3_wgrad_auto = _switch("CONV3X3_WGRAD_AUTO", "conv3x3_wgrad_auto")


CONV3X3_WGRAD_F32 = False   # the weight gradient of an eligible fp32 3x3 convolution outside autocast (conv3x3_f32_applies: the
#                             recipe of resnet/train.py:397-409) comes from mrla_conv3x3_f32_wgrad -- the fixed split and
#                             summation order of mrla_conv3x3_wgrad on the exact fp32-input MFMA, no atomics: a function of
#                             its arguments, eagerly and from a replayed graph, where the stock library's find mode picks an
#                             fp32 split-K solver that accumulates with atomics into a zero-filled buffer.  Forward
#                             and input gradient stay the stock operator's.  False (the default): conv(x) itself, the very
#                             same autograd graph and launches as before; conv3x3_wgrad_f32() turns it on for a block of
#                             code, reproducible_gradients() together with the 16-bit switches.  CONV3X3_WGRAD and
#                             CONV3X3_WGRAD_AUTO never route fp32.  Nothing is routed by shape: profiles/conv3x3_wgrad_f32.md
#                             has the numbers a default would rest on.


conv3x3_wgrad_f32 = _switch("CONV3X3_WGRAD_F32", "conv3x3_wgrad_f32")


CONV3X3_FWD = False   # the forward of an eligible 3x3 convolution (conv3x3_fwd_applies: the bottleneck's conv2, both of the basic
#                       block's; inference and frozen stages included) comes from mrla_conv3x3_fwd -- one fixed summation order,
#                       no split of the reduction: a function of its inputs alone, where the stock operator's output differs
#                       from run to run -- and so does its input gradient at stride 1 (the same kernel on the flipped,
#                       transposed weight); in front of a train-mode BatchNorm the kernel hands over the moment records and
#                       the separate moments pass over its output is gone (conv3x3_bn_act).  The stride-2 input gradient
#                       is the stock operator's unless CONV3X3_DGRAD is on as well.  False (the default): the very same
#                       autograd graph and launches as before; conv3x3_fwd() turns it on for a block of code.
#                       profiles/conv3x3_fwd.md has the numbers a change of the default rests on.


conv3x3_fwd = _switch("CONV3X3_FWD", "conv3x3_fwd")


CONV3X3_DGRAD = False   # the input gradient of an eligible stride-2 3x3 convolution (conv3x3_dgrad_applies: conv2 of the first
#                         bottleneck of stages 2-4, the first convolution of the same basic blocks) comes from
#                         mrla_conv3x3_dgrad_s2 -- four parity classes per 2x2 cell of dx, nine taps, all of n in one fixed
#                         order on the forward's own weight: a function of its inputs alone, where the stock operator's
#                         solver choice is not.  On its own: the stock forward and the stock weight gradient around it; with
#                         CONV3X3_FWD and CONV3X3_WGRAD no product of a 3x3 call site is left to the stock library.  False
#                         (the default): the very same autograd graph and launches as before; conv3x3_dgrad() turns it on
#                         for a block of code.  profiles/conv3x3_dgrad.md has the numbers a change of the default rests on.


conv3x3_dgrad = _switch("CONV3X3_DGRAD", "conv3x3_dgrad")


CONV3X3_DGRAD_FLIP = True   # the input gradient of an eligible stride-1 3x3 convolution inside a model's forward (a Conv3x3Bank in
#                             the bookkeeping scope), at a shape mrla_conv3x3_dgrad_flip_preferred answers 1 for (the large-batch
#                             steps: profiles/conv3x3_dgrad_flip.md), is the stock FORWARD convolution of dy with the flipped,
#                             transposed weight instead of the stock backward-data solver and the zero-fill of dX in front of
#                             it.  The bank keeps that weight and the forward's 16-bit copy for all routed convolutions with
#                             one launch per forward (mrla_conv3x3_weight_bank_refresh): no autocast cast kernel per
#                             convolution either.  Forward values and the weight gradient are bit for bit what they were; dX
#                             is the same sums from another solver.  False -- and every shape the rule answers 0 for, and every
#                             call outside a model -- the very same autograd graph and launches as before;
#                             conv3x3_dgrad_flip(False) turns it off for a block of code.


conv3x3_dgrad_flip = _switch("CONV3X3_DGRAD_FLIP", "conv3x3_dgrad_flip")


STEM_WGRAD = False   # the weight gradient of the stem's 7x7 / stride 2 convolution of three channels (stem_conv_applies: conv1 of
#                      ResNet_mrlal) comes from mrla_stem_conv_wgrad -- fixed split, fixed summation order, no atomics --
#                      written straight as the fp32 master weight's gradient.  The forward stays the stock operator's; the
#                      image batch needs no gradient.  False (the default): conv(x) itself, the very same autograd graph and
#                      launches as before; stem_wgrad() turns it on for a block of code.  profiles/stem_wgrad.md has the
#                      numbers a change of the default rests on.


stem_wgrad = _switch("STEM_WGRAD", "stem_wgrad")


STEM_WGRAD_F32 = False   # the weight gradient of the same convolution of an fp32 input outside autocast (stem_conv_f32_applies:
#                          the recipe of resnet/train.py:397-409) comes from mrla_stem_conv_f32_wgrad -- the fixed split and
#                          summation order of mrla_stem_conv_wgrad on the exact fp32-input MFMA, no atomics: a function of its
#                          arguments, eagerly and from a replayed graph.  The forward stays the stock operator's.  False (the
#                          default): conv(x) itself, the very same autograd graph and launches as before; stem_wgrad_f32()
#                          turns it on for a block of code, reproducible_gradients() together with the other three switches.
#                          STEM_WGRAD never routes fp32, STEM_WGRAD_F32 never routes 16-bit.  profiles/stem_wgrad_f32.md has
#                          the numbers a default would rest on.


stem_wgrad_f32 = _switch("STEM_WGRAD_F32", "stem_wgrad_f32")


@contextlib.contextmanager
def reproducible_gradients(enabled=True):
    """CONV3X3_WGRAD, CONV3X3_WGRAD_F32, STEM_WGRAD and STEM_WGRAD_F32 = `enabled` inside the block: with them on no weight
    gradient of a bf16 or fp16 resnet*_mrlal step is left to an atomic split-K solver, and none of an fp32 step (no autocast)
    either: the 3x3 gradients come from mrla_conv3x3_f32_wgrad and the stem's 7x7 gradient from mrla_stem_conv_f32_wgrad (the
    1x1 GEMMs' under fp32_gemms()).  The previous values come back on exit, also when the block raises."""
    with conv3x3_wgrad(enabled), conv3x3_wgrad_f32(enabled), stem_wgrad(enabled), stem_wgrad_f32(enabled):
        yield


WGRAD_BN_DX = True  # where the call site asks for it (conv_bn_act(..., fuse_dx=True): the bottleneck's conv3 and downsample) and
#                      one workgroup tile of that GEMM covers all channels of both sides (n = 256, k = 64: stage 1), it forms the convolution's input gradient dx = dy w as well (mrla_conv1x1_wgrad_bn_dx):
#                      dy, the largest tensor of the block, is neither written nor read back, and the input-gradient GEMM's
#                      launch is gone.  False: mrla_conv1x1_wgrad_bn and the input-gradient GEMM -- the same values bit for bit,
#                      kept for A/B runs and tests (and what a frozen input, a shortcut gradient arriving or any other shape
#                      get either way).


CHANNEL_GATE = True   # a BatchNorm2d followed by channel attention (SE or ECA: resnet_mrla_light.py:77-81,105-108) is one autograd
#                       node on the HIP passes of bn_gate_nhwc.hip: 3 passes over the activation forward and 5 backward, the
#                       BatchNorm's output never stored (bn_gate).  False: bn_act, then the eager se_layer / eca_layer modules --
#                       the same mathematics, kept for A/B runs and tests (and what NCHW tensors, both gates at once, another
#                       norm layer or an active KernelTimer get either way).


EVAL_FOLD = True  # a 1x1 GEMM convolution in front of an eval-mode BatchNorm2d (+ReLU), where nothing will be differentiated
#                   (inference; the frozen first stage of the detection backbone), is ONE launch: the GEMM applies the
#                   BatchNorm's fixed affine to its rounded product on the way out (mrla_conv1x1_fwd_affine) -- no apply pass,
#                   no convolution-output-sized temporary.  False: the two launches, the same values bit for bit, kept for
#                   A/B runs and tests.


def _seq():
    return SEQUENCES and TIMER is None


def _call(name, nbytes, *args, entry=None, alg=None, path=0):
    """Launch the C-ABI entry point `entry` (default: `name`); `name` is the label the optional timer records it under,
    with `nbytes` / `alg` / `path` as KernelTimer.summary describes them."""
    t = TIMER
    if t is not None and (t.names is None or name in t.names):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.call(entry or name, *args)
        e1.record()
        t.records.append((name, nbytes, e0, e1, alg, path))
    else:
        L.call(entry or name, *args)


def _ptr(t):
    """Device address as a plain int (ctypes converts it for a void* parameter; None is NULL) -- a c_void_p object per
    argument costs ~0.3 us on a path that passes ~6000 pointers per training step."""
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------------------
# Per-forward batching of the tiny bookkeeping kernels: 85 `num_batches_tracked += 1` launches and 16 x 4 stochastic-depth
# mask kernels per resnet50_mrlal step become one _foreach_add_ and one mask table.
# ------------------------------------------------------------------------------------------------------
class _Bookkeeping:
    def __init__(self, n_drop_paths, bank=None, bank3=None):
        self.counters, self.n_dp, self.table, self.key, self.next = [], int(n_drop_paths), None, None, 0
        self.bank = bank           # WeightBank of the model this forward belongs to (or None)
        self.bank3 = bank3         # its Conv3x3Bank (or None), refreshed by the first routed convolution of this forward
        self.bank3_fresh = False

    def drop_path_row(self, batch, drop_prob, device):
        """floor(keep + U[0,1)) / keep for one block: a row of a table drawn once per forward."""
        key = (batch, float(drop_prob), str(device))
        if self.table is None or self.key != key or self.next >= self.n_dp:
            keep = 1.0 - drop_prob
            self.table = torch.floor(keep + torch.rand((self.n_dp, batch), dtype=torch.float32, device=device)) / keep
            self.key, self.next = key, 0
        row = self.table[self.next]
        self.next += 1
        return row


_TLS = threading.local()


def current_bookkeeping():
    return getattr(_TLS, "book", None)


@contextlib.contextmanager
def batched_bookkeeping(n_drop_paths=0, bank=None, bank3=None):
    """Inside: train-mode BatchNorm counters handled by bn_act / the fused tails are collected and bumped with ONE
    torch._foreach_add_ on exit, layers.drop_path_scale serves stochastic-depth rows from one table, conv_bn_act
    takes the 16-bit working copies of its weights from `bank` (a refreshed WeightBank), and conv3x3 those of the routed
    3x3 convolutions from `bank3` (a Conv3x3Bank, which it refreshes once in here)."""
    prev, book = current_bookkeeping(), _Bookkeeping(n_drop_paths, bank, bank3)
    _TLS.book = book
    try:
        yield book
    finally:
        _TLS.book = prev
        if book.counters:
            torch._foreach_add_(book.counters, 1)


def bump_batch_counter(bn):
    """num_batches_tracked += 1 for a train-mode BatchNorm; returns the momentum to use (handles momentum=None)."""
    momentum = bn.momentum
    if bn.num_batches_tracked is not None:
        book = current_bookkeeping()
        if book is not None and momentum is not None:
            book.counters.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)
            if momentum is None:
                momentum = 1.0 / float(bn.num_batches_tracked)
    return momentum


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_graph_task = getattr(torch._C, "_current_graph_task_id", None)


def _graph_task_id():
    """Id of the autograd engine's running backward pass, -1 outside one (or when this torch has no such query)."""
    return _graph_task() if _graph_task is not None else -1


def _stream():
    """The current stream of the current device as the C ABI takes it (the raw-handle query: torch.cuda.current_stream()
    builds a Stream object, ~10 us on a path that launches ~600 kernels per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _f32(t):
    """Parameters / statistics as contiguous float32 (no copy when they already are)."""
    if t is None:
        return None
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _grad_like(g, shape, stride):
    """`g` (any dense tensor with shape.numel() elements in row-major order of `shape`) as a gradient with the
    parameter's own shape AND strides -- autograd's / DDP's gradient layout contract.  Free (a re-striding view) when the
    parameter's strides enumerate its elements in row-major order once size-1 dimensions are ignored (contiguous
    weights, and channels_last [n, k, 1, 1] / [c, 1, 3, 3] ones); any other dense layout gets a strided copy."""
    g = g.contiguous()
    dims = [(n, s) for n, s in zip(shape, stride) if n > 1]
    expect, row_major = 1, True
    for n, s in reversed(dims):
        row_major &= s == expect
        expect *= n
    if row_major:
        return g.as_strided(shape, stride)
    return torch.empty_strided(shape, stride, dtype=g.dtype, device=g.device).copy_(g.view(shape))


def _on_device(fn, at=1):
    """Run a Function.forward / backward body (or, with at=0, a plain function of a tensor) with the device of its tensor
    argument `at` current: the C ABI launches on the current HIP device and on the stream handed over, while the buffers
    live on x.device (a model on cuda:1 in a process whose current device is cuda:0 would otherwise launch on the wrong
    device)."""
    @functools.wraps(fn)
    def wrapped(*args):
        x = args[at]
        if isinstance(x, torch.Tensor) and x.is_cuda and x.device.index != torch.cuda.current_device():
            with torch.cuda.device(x.device):
                return fn(*args)
        return fn(*args)
    return wrapped


class _RunningStats:
    """running_mean / running_var as the contiguous float32 buffers the kernels read and (train mode) update in place.
    Buffers of another dtype or layout (model.half() / .bfloat16(), as the reference tolerates) go through float32 copies
    that are written back after the update; a wrong size raises."""

    def __init__(self, rm, rv, c, what):
        for t in (rm, rv):
            if t is None or not t.is_cuda or t.numel() != c:
                raise L.MrlaHipError(f"{what}: running statistics must be CUDA tensors with {c} elements")
        self.src = (rm, rv)
        ok = all(t.dtype == torch.float32 and t.is_contiguous() for t in (rm, rv))
        self.rm, self.rv = (rm, rv) if ok else (rm.detach().float().contiguous(), rv.detach().float().contiguous())
        self.copy_back = not ok

    def finish(self, updated):
        if self.copy_back and updated:
            with torch.no_grad():
                self.src[0].copy_(self.rm)
                self.src[1].copy_(self.rv)


def _is_fused_bn(bn):
    """An nn.BatchNorm2d with affine parameters and tracked statistics: the norm layer the fused passes stand in for."""
    return type(bn) is torch.nn.BatchNorm2d and bn.affine and bn.track_running_stats


def _bn_step(bn):
    """(training, momentum) of this forward of the BatchNorm module `bn`; in train mode its batch counter is bumped
    (bump_batch_counter, which also resolves momentum=None).  An eval-mode momentum of None is 0.0: nothing reads it."""
    training = bn.training
    momentum = bump_batch_counter(bn) if training else bn.momentum
    return training, momentum or 0.0


class _BnForward:
    """What the forward of a node with a BatchNorm hands its statistics pass: gamma / beta as float32, the running statistics
    (_RunningStats) and bnbuf [4, c] = scale | shift | saved mean | saved 1/sigma, which that pass fills."""
    __slots__ = ("gamma32", "beta32", "rs", "bnbuf", "mode", "momentum", "eps")

    def __init__(self, gamma, beta, running_mean, running_var, c, mode, momentum, eps, dev, what):
        self.gamma32, self.beta32 = _f32(gamma), _f32(beta)
        self.rs = _RunningStats(running_mean, running_var, c, what)
        self.bnbuf = torch.empty((4, c), dtype=torch.float32, device=dev)
        self.mode, self.momentum, self.eps = mode, float(momentum), float(eps)

    def stats(self, amom, pivot, rows, c, count, st):
        """mrla_bn_stats_fwd on `rows` partial (sum, sum^2) rows of `count` pixels each (about `pivot` where given)."""
        bb = self.bnbuf
        _call("mrla_bn_stats_fwd", 0, _ptr(amom), _ptr(pivot), _ptr(self.gamma32), _ptr(self.beta32), _ptr(self.rs.rm),
              _ptr(self.rs.rv), self.mode, self.momentum, self.eps, _ptr(bb[0]), _ptr(bb[1]), _ptr(bb[2]), _ptr(bb[3]), rows, c,
              count, st)

    def stats_rows(self, records, rows, c, st):
        """mrla_bn_stats_fwd_rows on the `rows` pivoted moment records a producer GEMM left (train mode only)."""
        bb = self.bnbuf
        _call("mrla_bn_stats_fwd_rows", 0, _ptr(records), _ptr(self.gamma32), _ptr(self.beta32), _ptr(self.rs.rm),
              _ptr(self.rs.rv), L.BN_TRAIN, self.momentum, self.eps, _ptr(bb[0]), _ptr(bb[1]), _ptr(bb[2]), _ptr(bb[3]), rows, c, st)

    def finish(self):
        self.rs.finish(self.mode == L.BN_TRAIN)


class _BnBackward:
    """The per-channel constants of a BatchNorm backward: small [5, c] = cb[c, 3] | dgamma | dbeta.  A sequence entry point
    takes `small` whole; stats() is the per-pass form and returns the cb view the apply pass reads."""
    __slots__ = ("small",)

    def __init__(self, c, dev):
        self.small = torch.empty((5, c), dtype=torch.float32, device=dev)

    def stats(self, tmom, gamma32, bnbuf, mode, centered, rows, c, count, st):
        """mrla_bn_stats_bwd on `rows` partial (sum dz, sum dz*x) rows of `count` pixels each; centered: the second sum is
        about the saved mean."""
        s = self.small
        cb = s[:3].view(c, 3)
        _call("mrla_bn_stats_bwd", 0, _ptr(tmom), _ptr(gamma32), _ptr(bnbuf[2]), _ptr(bnbuf[3]), mode, centered, _ptr(cb),
              _ptr(s[3]), _ptr(s[4]), rows, c, count, st)
        return cb

    def grads(self, dtype):
        """(dgamma, dbeta) in the parameters' dtype."""
        return self.small[3].to(dtype), self.small[4].to(dtype)


def _require_cuda(x, what):
    if not x.is_cuda:
        raise L.MrlaHipError(f"{what}: got a {x.device} tensor. mrla_amd runs only on an AMD GPU through libmrla_hip.so; "
                             "the CPU restatement lives in oracle/ and is test infrastructure, not a fallback.")
    if x.dtype not in _DT:
        raise L.MrlaHipError(f"{what}: unsupported dtype {x.dtype}")


_CL = torch.channels_last


def _layout_of(x, want=None):
    """(layout enum, tensor to hand to the kernels).  NCHW-contiguous is the reference's contract; channels_last
    (NHWC) tensors run on the NHWC kernels without any conversion.  `want` forces the layout of a second operand."""
    if want is None:
        if x.is_contiguous():
            return L.NCHW, x
        if x.dim() == 4 and x.is_contiguous(memory_format=_CL):
            return L.NHWC, x
        return L.NCHW, x.contiguous()
    if want == L.NHWC:
        return L.NHWC, x.contiguous(memory_format=_CL)
    return L.NCHW, x.contiguous()


class _DeferredBnBox:
    """Hand-over between the fused MRLA producer and the deferred BatchNorm in front of it (bn_act(defer=True)): the MRLA
    backward apply pass forms dpre, the gradient of that BatchNorm's output, and can take the two per-channel sums its
    backward needs on the way (mrla_light_apply_bwd: pre / pre_tmom).  It leaves them here, tagged with the gradient tensor
    they belong to; the BatchNorm's backward uses them when exactly that tensor arrives, and runs its own statistics pass
    otherwise (another consumer added to the gradient, a layout conversion, a path without the fused sums)."""
    __slots__ = ("ptr", "shape", "tmom", "rows", "center", "ref", "version")

    def __init__(self):
        self.ptr = self.shape = self.tmom = self.rows = self.ref = self.version = None
        self.center = None         # that BatchNorm's saved mean [c]: the sums are taken about it

    def put(self, dpre, tmom, rows):
        if (dpre.numel() // dpre.shape[1]) % rows:       # the BatchNorm backward takes rows of equally many pixels: fold them
            tmom, rows = tmom.sum(0, keepdim=True, dtype=torch.float64).float(), 1
        self.ptr, self.shape, self.tmom, self.rows = dpre.data_ptr(), tuple(dpre.shape), tmom, rows
        self.ref, self.version = weakref.ref(dpre), dpre._version

    def take(self, dy):
        """The sums belong to `dy` only if it is the very tensor the producer wrote, unmodified: the producer's tensor is
        still alive (so nothing else can have been allocated at its address), `dy` sits at that address with that shape,
        and nothing has been written into it since (autograd accumulates a second consumer's gradient IN PLACE into the
        first-arrived buffer when it owns it; a tensor hook may edit it: both bump the version counter)."""
        alive = self.ref() if self.ref is not None else None
        ok = (self.tmom is not None and alive is not None and dy.data_ptr() == self.ptr and tuple(dy.shape) == self.shape
              and dy._version == self.version)
        tmom, rows = self.tmom, self.rows
        self.ptr = self.shape = self.tmom = self.rows = self.ref = self.version = None
        return (tmom, rows) if ok else None


class LightConfig:
    """Static configuration of one MRLA-light call.  fuse: the first tensor argument is the block's pre-activation
    and x_t = relu(pre + o_prev) is formed inside the statistics kernel (resnet_mrla_light.py:113-114 folded in)."""
    __slots__ = ("d", "bn_mode", "momentum", "eps", "res", "act", "fuse", "pre_affine", "pre_box", "infer")

    def __init__(self, d, bn_mode=L.BN_NONE, momentum=0.1, eps=1e-5, res=0, act=L.ACT_NONE, fuse=False, pre_affine=None,
                 pre_box=None):
        self.d, self.bn_mode, self.momentum, self.eps, self.res, self.act = d, bn_mode, momentum, eps, res, act
        self.pre_affine = pre_affine     # (scale[c], shift[c]) fp32 of a deferred BatchNorm in front of the fused producer
        self.pre_box = pre_box           # its _DeferredBnBox: where the backward leaves that BatchNorm's gradient sums
        self.infer = False               # nothing will be differentiated (set by mrla_light from the autograd state)
        self.fuse = fuse


class _LightFn(torch.autograd.Function):
    """out = res*x + dp[b] * BN( a[b,g] * act(dwconv3x3(x, wv)) + lam * o_prev )

    Covers mrla_light_layer (o_prev = lam = BN = dp = None, res = 0), the light mrla_module (+ lam*o_prev)
    and the fused block tail of resnet_mrla_light.py:116 (BN + DropPath + residual).
    """

    @staticmethod
    @_on_device
    def forward(ctx, x, o_prev, wq, wk, wv, lam, gamma, beta, running_mean, running_var, dp, cfg):
        _require_cuda(x, "mrla light forward")
        layout, xc = _layout_of(x)
        b, c, h, w = xc.shape
        d = cfg.d
        # NCHW is the reference's contract for any map size (mmdet: 800x1333); the NCHW slab kernels need a plane row to
        # fit one wave and a slab to fit the LDS.  Shapes beyond that run on the NHWC kernels through ONE internal
        # channels_last conversion, and the result goes back to NCHW-contiguous memory.
        via_nhwc = layout == L.NCHW and L.load().mrla_light_wgrad_rows(b, c, h, w, _DT[xc.dtype], L.NCHW) == L.EUNSUPPORTED
        if via_nhwc:
            layout, xc = L.NHWC, xc.contiguous(memory_format=_CL)
        if c % d:
            raise L.MrlaHipError(f"channels ({c}) not divisible by dim_perhead ({d})")
        oc = None
        if o_prev is not None:
            if o_prev.shape != x.shape or o_prev.dtype != x.dtype:
                raise L.MrlaHipError("o_prev must match x in shape and dtype")
            oc = _layout_of(o_prev, layout)[1]
        dt = _DT[xc.dtype]
        dev = xc.device
        wq32, wk32 = _f32(wq).reshape(-1), _f32(wk).reshape(-1)
        wv32 = _f32(wv).reshape(c, 9)
        lam32 = _f32(lam).reshape(-1) if lam is not None else None
        dp32 = _f32(dp).reshape(-1) if dp is not None else None
        ks = wq32.numel()
        G = c // d
        st = _stream()

        # (the statistics passes leave one record per strip range and fold them into mom[0]; > 1 range only for few, large images)
        msplits = L.load().mrla_light_mom_splits(b, c, h, w, dt, layout)
        L.check(min(msplits, 0), "mrla_light_mom_splits")
        mom = torch.empty((msplits, b, c, L.FWD_MOMENTS), dtype=torch.float32, device=dev)
        if cfg.fuse and (oc is None or cfg.act != L.ACT_NONE):
            raise L.MrlaHipError("the fused relu(pre + o_prev) producer needs o_prev and no activation on V")
        nb = xc.numel() * xc.element_size()
        # inference form: nothing will be differentiated and bn_mrla does not need the batch statistics of m, so x_t is
        # neither materialised nor saved (pooling pass + an apply pass that re-forms x_t: 5N instead of 6N elements)
        infer = cfg.fuse and layout == L.NHWC and cfg.bn_mode != L.BN_TRAIN and c % 64 == 0 and cfg.infer
        # x_t = relu(bn3(pre) + o_prev) is re-formed by every pass that needs it instead of being stored (ABI 5)
        lean = bool(not infer and LEAN and cfg.fuse and not via_nhwc
                    and L.load().mrla_light_lean_supported(b, c, h, w, dt, layout) == 1)
        pre = psc = psh = None
        if cfg.fuse:
            pre, xc = xc, (None if (lean or infer) else torch.empty_like(xc))
            psc, psh = cfg.pre_affine if cfg.pre_affine is not None else (None, None)
        gate = torch.empty((b, G), dtype=torch.float32, device=dev)
        bn = bnbuf = gamma32 = None
        if cfg.bn_mode != L.BN_NONE:
            bn = _BnForward(gamma, beta, running_mean, running_var, c, cfg.bn_mode, cfg.momentum, cfg.eps, dev,
                            "mrla light forward")
            bnbuf, gamma32 = bn.bnbuf, bn.gamma32
        out = torch.empty_like(oc if lean else pre if infer else xc)
        if not infer and _seq():
            L.call("mrla_light_tail_fwd", _ptr(pre if cfg.fuse else xc), _ptr(psc), _ptr(psh), _ptr(oc), _ptr(wq32), _ptr(wk32),
                   ks, _ptr(wv32), _ptr(lam32), _ptr(gamma32), _ptr(bn.beta32) if bn is not None else None,
                   _ptr(bn.rs.rm) if bn is not None else None, _ptr(bn.rs.rv) if bn is not None else None, cfg.bn_mode,
                   float(cfg.momentum), float(cfg.eps), _ptr(dp32), _ptr(mom), _ptr(xc) if (cfg.fuse and not lean) else None,
                   _ptr(gate), _ptr(bnbuf), _ptr(out), b, c, h, w, d, cfg.res, (2 if lean else int(cfg.fuse)), dt, layout,
                   cfg.act, st)
        else:                       # one call per pass (the inference form has no sequence entry point)
            if infer:
                rows = L.load().mrla_bn_moment_rows(b, c, h, w, layout)
                part = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
                _call("mrla_light_pool_fused", nb * 2, _ptr(pre), _ptr(psc), _ptr(psh), _ptr(oc), _ptr(part), _ptr(mom), b, c, h,
                      w, dt, layout, st)
            elif cfg.fuse:
                _call("mrla_light_stats_fwd_fused", nb * (2 if lean else 3), _ptr(pre), _ptr(psc), _ptr(psh),
                      _ptr(oc), _ptr(wv32), _ptr(mom), _ptr(xc), b, c, h, w, dt, layout, st)
            else:
                _call("mrla_light_stats_fwd", nb * (2 if oc is not None else 1), _ptr(xc), _ptr(oc), _ptr(wv32), _ptr(mom), b, c,
                      h, w, dt, layout, cfg.act, st)
            _call("mrla_light_gate_fwd", 0, _ptr(mom), _ptr(wq32), _ptr(wk32), ks, _ptr(gate), b, c, h * w, d, st)
            sc = sh = None
            if bn is not None:
                _call("mrla_light_bn_fwd", 0, _ptr(mom), _ptr(gate), _ptr(lam32), _ptr(gamma32), _ptr(bn.beta32), _ptr(bn.rs.rm),
                      _ptr(bn.rs.rv), cfg.bn_mode, bn.momentum, bn.eps, _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(bnbuf[2]),
                      _ptr(bnbuf[3]), b, c, h * w, d, st)
                sc, sh = _ptr(bnbuf[0]), _ptr(bnbuf[1])
            if lean or infer:       # the apply pass that re-forms x_t from pre
                _call("mrla_light_apply_fwd_fused", nb * 3, _ptr(pre), _ptr(psc), _ptr(psh), _ptr(oc), _ptr(wv32), _ptr(gate), sc,
                      sh, _ptr(lam32), _ptr(dp32), _ptr(out), b, c, h, w, d, cfg.res, dt, layout, st, path=nb * 3)
            else:
                _call("mrla_light_apply_fwd", nb * (3 if oc is not None else 2), _ptr(xc), _ptr(oc), _ptr(wv32), _ptr(gate),
                      sc, sh, _ptr(lam32), _ptr(dp32), _ptr(out), b, c, h, w, d, cfg.res, dt, layout, cfg.act, st,
                      path=nb * (3 if oc is not None else 2))
        if infer:                   # (nothing is saved: there is no backward)
            return out.contiguous() if via_nhwc else out
        if bn is not None:
            bn.finish()

        ctx.cfg, ctx.layout, ctx.ks = cfg, layout, ks
        ctx.shapes = (wq.shape, wk.shape, wv.shape, lam.shape if lam is not None else None)
        ctx.wv_stride = wv.stride()          # gradient layout contract of DDP: same strides as the parameter
        ctx.pdtypes = (wq.dtype, wk.dtype, wv.dtype, lam.dtype if lam is not None else None,
                       gamma.dtype if gamma is not None else None)
        # conv3's raw output, when the BatchNorm behind it was deferred and its backward sums can ride in apply_bwd
        keep_pre = (cfg.fuse and cfg.pre_box is not None and not via_nhwc
                    and L.load().mrla_light_apply_bwd_pre_sums(b, c, h, w, dt, layout) == 1)
        ctx.lean, ctx.pre_sums = lean, keep_pre
        psc, psh = cfg.pre_affine if (lean and cfg.pre_affine is not None) else (None, None)
        ctx.save_for_backward(xc, oc, wq32, wk32, wv32, lam32, gamma32, dp32, mom, gate, bnbuf,
                              pre if (keep_pre or lean) else None, psc, psh)
        return out.contiguous() if via_nhwc else out

    @staticmethod
    @_on_device
    def backward(ctx, dout):
        xc, oc, wq32, wk32, wv32, lam32, gamma32, dp32, mom, gate, bnbuf, pre, psc, psh = ctx.saved_tensors
        cfg, layout, ks, lean = ctx.cfg, ctx.layout, ctx.ks, ctx.lean
        like = oc if lean else xc                    # (lean: x_t was never stored; it is re-formed from pre, psc, psh, oc)
        b, c, h, w = like.shape
        d = cfg.d
        dt = _DT[like.dtype]
        dev = like.device
        st = _stream()
        nb = like.numel() * like.element_size()
        if dout.dtype != like.dtype:
            dout = dout.to(like.dtype)
        dout = _layout_of(dout, layout)[1]

        has_bn = cfg.bn_mode != L.BN_NONE
        # (partial records of the backward statistics pass: > 1 only for few, large images -- detection batches)
        splits = L.load().mrla_light_bmom_splits(b, c, h, w, dt, layout)
        L.check(min(splits, 0), "mrla_light_bmom_splits")
        bmom = torch.empty((splits, b, c, L.BWD_MOMENTS), dtype=torch.float32, device=dev)
        small = torch.empty((11, c), dtype=torch.float32, device=dev)     # cb[c,4] | dgamma | dbeta | dlam | cb_lo[c,4]
        dyx = torch.empty((b, c), dtype=torch.float32, device=dev)
        dwqk_part = torch.empty((b, 2 * ks), dtype=torch.float32, device=dev)
        rows = L.load().mrla_light_wgrad_rows(b, c, h, w, dt, layout)
        L.check(min(rows, 0), "mrla_light_wgrad_rows")
        dwv_part = torch.empty((rows, c * 9), dtype=torch.float32, device=dev)
        dx = torch.empty_like(like)
        do = torch.empty_like(oc) if oc is not None else None
        # the deferred bn3's backward sums (sum dpre, sum dpre*y3) ride in the apply pass: one more row fetch, no 2N pass
        pre_tmom = center = None
        if ctx.pre_sums and pre is not None:
            pre_tmom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
            center = _ptr(cfg.pre_box.center)
        elif not lean:
            pre = None
        wsum = torch.empty((c * 9 + 2 * ks,), dtype=torch.float32, device=dev)
        if _seq():
            L.call("mrla_light_tail_bwd", _ptr(dout), _ptr(xc), _ptr(oc), _ptr(wq32), _ptr(wk32), ks, _ptr(wv32), _ptr(lam32),
                   _ptr(gamma32) if has_bn else None, _ptr(dp32), _ptr(mom), _ptr(gate), _ptr(bnbuf) if has_bn else None,
                   cfg.bn_mode, _ptr(bmom), _ptr(small), _ptr(dyx), _ptr(dwqk_part), _ptr(dwv_part), rows, _ptr(dx), _ptr(do),
                   _ptr(pre), _ptr(psc), _ptr(psh), center, _ptr(pre_tmom), _ptr(wsum), b, c, h, w, d, cfg.res, int(cfg.fuse),
                   dt, layout, cfg.act, st)
        else:
            if lean:
                _call("mrla_light_stats_bwd_fused", nb * 3, _ptr(dout), _ptr(pre), _ptr(psc), _ptr(psh), _ptr(oc), _ptr(wv32),
                      _ptr(mom), _ptr(bmom), b, c, h, w, dt, layout, st)
            else:
                _call("mrla_light_stats_bwd", nb * (3 if oc is not None else 2), _ptr(dout), _ptr(xc), _ptr(oc), _ptr(wv32),
                      _ptr(mom), _ptr(bmom), b, c, h, w, dt, layout, cfg.act, st)
            cb, cb_lo = small[:4].view(c, 4), small[7:].view(c, 4)
            _call("mrla_light_bn_bwd", 0, _ptr(mom), _ptr(bmom), _ptr(gate), _ptr(lam32), _ptr(gamma32) if has_bn else None,
                   _ptr(dp32), _ptr(bnbuf[2]) if has_bn else None, _ptr(bnbuf[3]) if has_bn else None, cfg.bn_mode,
                   _ptr(cb), _ptr(cb_lo), _ptr(small[4]) if has_bn else None, _ptr(small[5]) if has_bn else None,
                   _ptr(small[6]) if lam32 is not None else None, b, c, h * w, d, st)
            _call("mrla_light_gate_bwd", 0, _ptr(mom), _ptr(bmom), _ptr(gate), _ptr(cb), _ptr(cb_lo), _ptr(dp32), _ptr(wq32),
                   _ptr(wk32), ks, _ptr(dyx), _ptr(dwqk_part), b, c, h * w, d, st)
            if lean:
                # dOut, y3, o_prev in; dx, do out: section 8(d)'s five passes exactly (x_t is re-formed, bn3's sums ride along)
                _call("mrla_light_apply_bwd", nb * 5, _ptr(dout), _ptr(pre), _ptr(psc), _ptr(psh), _ptr(oc), _ptr(wv32),
                      _ptr(gate), _ptr(cb), _ptr(lam32), _ptr(dp32), _ptr(dyx), _ptr(dx), _ptr(do), _ptr(dwv_part),
                      center, _ptr(pre_tmom), b, c, h, w, d, cfg.res, dt, layout, st, entry="mrla_light_apply_bwd_fused",
                      alg=nb * 5, path=nb * 5)
            else:
                _call("mrla_light_apply_bwd", nb * ((5 if oc is not None else 3) + (pre is not None)),
                      _ptr(dout), _ptr(xc), _ptr(oc), _ptr(wv32), _ptr(gate), _ptr(cb), _ptr(lam32),
                      _ptr(dp32), _ptr(dyx), _ptr(dx), _ptr(do), _ptr(dwv_part), _ptr(pre), center, _ptr(pre_tmom), b, c, h, w,
                      d, cfg.res, int(cfg.fuse), dt, layout, cfg.act, st,
                      # section 8(d): dOut, x_t, o_prev in; dx, do out (the y3 row read for bn3's folded sums is not in that count)
                      alg=nb * (5 if oc is not None else 3), path=nb * (5 if oc is not None else 3))
            _call("mrla_reduce_rows2", 0, _ptr(dwv_part), _ptr(wsum), rows, c * 9, _ptr(dwqk_part), _ptr(wsum[c * 9:]), b, 2 * ks, st)
        if pre_tmom is not None:
            cfg.pre_box.put(dx, pre_tmom, rows)

        sq, sk, sv, sl = ctx.shapes
        tq, tk, tv, tl, tg = ctx.pdtypes
        dwv = _grad_like(wsum[:c * 9].to(tv), sv, ctx.wv_stride)
        dwq = wsum[c * 9:c * 9 + ks].view(sq).to(tq)
        dwk = wsum[c * 9 + ks:].view(sk).to(tk)
        dlam = small[6].view(sl).to(tl) if lam32 is not None else None
        dgamma = small[4].to(tg) if has_bn else None
        dbeta = small[5].to(tg) if has_bn else None
        return dx, do, dwq, dwk, dwv, dlam, dgamma, dbeta, None, None, None, None


def mrla_light(x, wq, wk, wv, d, o_prev=None, lam=None, bn=None, dp=None, res=False, act_gelu=False,
               pre_activation=False):
    """Functional entry point.

    bn: None or dict(weight, bias, running_mean, running_var, training, momentum, eps).
    dp: per-sample drop-path multiplier [b] (mask / keep_prob) or None.
    pre_activation: `x` is the block's pre-activation; x_t = relu(x + o_prev) is formed inside the kernels.  When `x`
    came out of `bn_act(..., defer=True)` its BatchNorm affine is applied there too (x then aliases the conv output).
    """
    pre_affine, pre_box = getattr(x, "_mrla_affine", None), getattr(x, "_mrla_bn_box", None)
    if pre_affine is not None and not pre_activation:
        raise L.MrlaHipError("a deferred BatchNorm output can only feed the fused producer (pre_activation=True)")
    tensors = [t for t in (x, o_prev, wq, wk, wv, lam) if t is not None]
    if bn is not None:
        tensors += [bn["weight"], bn["bias"]]
    infer = not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))
    mode, bnp = L.BN_NONE, {}
    if bn is not None:
        mode, bnp = (L.BN_TRAIN if bn["training"] else L.BN_EVAL), bn
    cfg = LightConfig(d, mode, bnp.get("momentum", 0.1), bnp.get("eps", 1e-5), int(res), L.ACT_GELU if act_gelu else L.ACT_NONE,
                      fuse=pre_activation, pre_affine=pre_affine, pre_box=pre_box)
    cfg.infer = infer
    return _LightFn.apply(x, o_prev, wq, wk, wv, lam, bnp.get("weight"), bnp.get("bias"), bnp.get("running_mean"),
                          bnp.get("running_var"), dp, cfg)


# ======================================================================================================
# MRLA-base
# ======================================================================================================
class BaseStage:
    """Stage-resident K/V history of MRLA-base on the device (replaces the reference's torch.cat growth).

    One instance lives for one forward(+backward) pass of one network stage: the `init_cell` layer creates
    it, every later layer of the stage appends one slot.  Gradients with respect to the history do not
    travel along autograd edges; they are accumulated in the dA / dK rings, which is valid because layer
    t+1's backward always runs before layer t's (x_{t+1} depends on out_t through the block chain).
    """

    def __init__(self, b, c, h, w, d, dtype, device, capacity, layout=L.NCHW):
        self.b, self.c, self.h, self.w, self.d = b, c, h, w, d
        self.dtype, self.device, self.layout = dtype, device, layout
        self.T = max(1, int(capacity))
        self.t = 0
        self.bwd_started = False
        self.bwd_task = -1        # autograd graph-task id of the backward pass the dA / dK rings currently belong to
        self.bwd_last_t = 0       # layer index of the previous backward call (calls of one pass come in decreasing t)
        self.bwd_top = 0          # deepest layer that took part in the current backward pass
        self.V = torch.empty(self._vshape(self.T), dtype=dtype, device=device)
        self.K = torch.empty((b, self.T, c), dtype=torch.float32, device=device)
        self.P = torch.empty((b, c // d, self.T, self.T), dtype=torch.float32, device=device)
        self.dA = self.dK = None

    @staticmethod
    def layout_for(x, d):
        """MRLA_NHWC when `x` is a channels_last tensor the slot-major NHWC kernels handle, else MRLA_NCHW."""
        if x.dim() == 4 and x.dtype in _DT:
            b, c, h, w = x.shape
            lib = L.load()
            nhwc_ok = lib.mrla_base_tile_rows(b, c, h, w, _DT[x.dtype], L.NHWC) > 0
            if not x.is_contiguous() and x.is_contiguous(memory_format=_CL) and nhwc_ok:
                return L.NHWC
            # channel-contiguous views that are not dense (DeiT's map tokens x[:, 1:] seen as [b, c, 14, 14]): one dense
            # NHWC copy is cheaper than the transposing copy the NCHW kernels would need
            if nhwc_ok and c > 1 and x.stride(1) == 1 and not x.is_contiguous():
                return L.NHWC
            # NCHW tensors the slab kernels cannot take (plane rows wider than a wave, slabs beyond the LDS) go through one
            # internal channels_last conversion per layer instead of failing (the reference accepts any map size)
            if nhwc_ok and lib.mrla_light_wgrad_rows(b, c, h, w, _DT[x.dtype], L.NCHW) == L.EUNSUPPORTED:
                return L.NHWC
        return L.NCHW

    def _vshape(self, T):
        """NCHW: [b, T, c, h, w] (the reference's V layout).  NHWC: slot-major [T, b, h, w, c]."""
        if self.layout == L.NHWC:
            return (T, self.b, self.h, self.w, self.c)
        return (self.b, T, self.c, self.h, self.w)

    def slot(self, ring, j):
        return ring[j] if self.layout == L.NHWC else ring[:, j]

    def reserve_slot(self):
        """Make room for one more layer (amortised doubling when the capacity hint was too small)."""
        if self.t < self.T:
            return
        if self.bwd_started:
            raise L.MrlaHipError("MRLA-base history grown after its backward pass started")
        T2, t = 2 * self.T, self.t
        V = torch.empty(self._vshape(T2), dtype=self.dtype, device=self.device)
        K = torch.empty((self.b, T2, self.c), dtype=torch.float32, device=self.device)
        P = torch.empty((self.b, self.c // self.d, T2, T2), dtype=torch.float32, device=self.device)
        if self.layout == L.NHWC:
            V[:t].copy_(self.V[:t])
        else:
            V[:, :t].copy_(self.V[:, :t])
        K[:, :t].copy_(self.K[:, :t])
        P[:, :, :t, :t].copy_(self.P[:, :, :t, :t])
        self.V, self.K, self.P, self.T = V, K, P, T2

    def begin_layer_backward(self, t):
        """Called by layer t's backward.  Returns True on the first call of a backward PASS: then the dK ring is re-zeroed
        and `bwd_top` (the deepest layer whose dA slot this pass fills) is reset.  A pass is identified by the autograd
        engine's graph-task id (a partial pass -- autograd.grad down to layer 3 -- followed by one whose deepest layer is
        shallower is a new pass although t decreased); outside an engine-driven backward (id -1) a pass is recognised
        by t not decreasing: a repeated backward over the same graph starts again at the top."""
        if self.dA is None:
            self.dA = torch.empty_like(self.V)
            self.dK = torch.empty_like(self.K)
        task = _graph_task_id()
        if task != -1:
            first = (not self.bwd_started) or task != self.bwd_task
        else:
            first = (not self.bwd_started) or t >= self.bwd_last_t
        self.bwd_started = True
        self.bwd_task = task
        self.bwd_last_t = t
        if first:
            self.bwd_top = t
        return first

    def views(self):
        """(K[b,t,c], V[b,t,c,h,w]) as the reference returns them -- views of the rings."""
        K = self.K[:, :self.t]
        V = self.V[:self.t].permute(1, 0, 4, 2, 3) if self.layout == L.NHWC else self.V[:, :self.t]
        K._mrla_stage = V._mrla_stage = self
        return K, V


class BaseConfig:
    __slots__ = ("d", "bn_mode", "momentum", "eps", "tail", "fuse", "pre_affine", "pre_box")

    def __init__(self, d, bn_mode=L.BN_NONE, momentum=0.1, eps=1e-5, tail=False, fuse=False, pre_affine=None, pre_box=None):
        self.d, self.bn_mode, self.momentum, self.eps, self.tail, self.fuse = d, bn_mode, momentum, eps, tail, fuse
        self.pre_affine = pre_affine     # deferred bn3 affine (NHWC stages only), see bn_act(defer=True)
        self.pre_box = pre_box           # its _DeferredBnBox: where the value backward leaves that BatchNorm's gradient sums


class _BaseFn(torch.autograd.Function):
    """tail:  out = x + dp[b]*relu(BN(attn)),  attn = sum_{j<=t} softmax_j(<q_t,k_j>/sqrt(d)) * v_j
    no tail: out = attn  (bare mrla_base_layer)."""

    @staticmethod
    @_on_device
    def forward(ctx, x, identity, wq, wk, wv, gamma, beta, running_mean, running_var, dp, stage, cfg):
        _require_cuda(x, "mrla base forward")
        layout, xc = _layout_of(x, stage.layout)    # the stage's rings fix the layout (NHWC rings are slot-major)
        b, c, h, w = xc.shape
        d = cfg.d
        if (b, c, h, w, d) != (stage.b, stage.c, stage.h, stage.w, stage.d) or xc.dtype != stage.dtype:
            raise L.MrlaHipError("input does not match the stage's K/V history (shape/dtype); is init_cell set on the "
                                 "first block of the stage?")
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        wq32, wk32 = _f32(wq).reshape(-1), _f32(wk).reshape(-1)
        wv32 = _f32(wv).reshape(c, 9)
        dp32 = _f32(dp).reshape(-1) if dp is not None else None
        ks = wq32.numel()
        stage.reserve_slot()
        t, T = stage.t + 1, stage.T

        # ([splits, b, c, 8]: mrla_light_stats_fwd* -- the NCHW path's pooling pass below -- may leave a record per strip range)
        mom = torch.empty((max(1, L.load().mrla_light_mom_splits(b, c, h, w, dt, layout)), b, c, L.FWD_MOMENTS), dtype=torch.float32,
                          device=dev)
        nhwc = layout == L.NHWC
        es = xc.element_size()
        idc = pre = None
        if cfg.fuse:                # x is the pre-activation: x_t = relu(x + identity) is formed by the pooling pass
            idc = _layout_of(identity, layout)[1]
            pre, xc = xc, torch.empty_like(xc)
        psc, psh = cfg.pre_affine if cfg.pre_affine is not None else (None, None)      # (NHWC stages only: mrla_base)
        q = torch.empty((b, c), dtype=torch.float32, device=dev)
        attn = torch.empty_like(xc)
        arows = L.load().mrla_base_tile_rows(b, c, h, w, dt, layout)      # rows of the (sum, sum^2) partials
        L.check(min(arows, 0), "mrla_base_tile_rows")
        amom = torch.empty((arows, c, 2), dtype=torch.float32, device=dev)
        bn = bnbuf = gamma32 = None
        out = attn
        if cfg.tail:
            bn = _BnForward(gamma, beta, running_mean, running_var, c, cfg.bn_mode, cfg.momentum, cfg.eps, dev,
                            "mrla base forward")
            bnbuf, gamma32 = bn.bnbuf, bn.gamma32
            out = torch.empty_like(xc)
        if nhwc and _seq():     # the whole layer + tail: one call (mrla_base_layer_fwd)
            L.call("mrla_base_layer_fwd", _ptr(pre if cfg.fuse else xc), _ptr(psc), _ptr(psh), _ptr(idc), _ptr(wq32),
                   _ptr(wk32), ks, _ptr(wv32), _ptr(gamma32), _ptr(bn.beta32) if bn is not None else None,
                   _ptr(bn.rs.rm) if bn is not None else None, _ptr(bn.rs.rv) if bn is not None else None,
                   cfg.bn_mode if cfg.tail else L.BN_NONE, float(cfg.momentum), float(cfg.eps), _ptr(dp32), _ptr(mom),
                   _ptr(xc) if cfg.fuse else None, _ptr(stage.V), _ptr(stage.K), _ptr(stage.P), _ptr(q), _ptr(attn), _ptr(amom),
                   arows, _ptr(bnbuf), _ptr(out) if cfg.tail else None, int(cfg.tail), b, c, h, w, d, T, t, dt, st)
        else:
            nb = xc.numel() * es
            if nhwc:                # one pass: pooling moments, V_t -> ring slot (and x_t = relu(x + identity) when fused)
                _call("mrla_base_pool_value_fwd", nb * (4 if cfg.fuse else 2), _ptr(pre if cfg.fuse else xc),
                      _ptr(psc), _ptr(psh), _ptr(idc), _ptr(wv32), _ptr(mom), _ptr(xc) if cfg.fuse else None,
                      _ptr(stage.V[t - 1]), b, c, h, w, dt, layout, st, path=nb * 2)
            elif cfg.fuse:
                _call("mrla_light_stats_fwd_fused", nb * 3, _ptr(pre), None, None, _ptr(idc),
                      _ptr(wv32), _ptr(mom), _ptr(xc), b, c, h, w, dt, layout, st)
            else:
                _call("mrla_light_stats_fwd", nb, _ptr(xc), None, _ptr(wv32), _ptr(mom), b, c, h,
                      w, dt, layout, L.ACT_NONE, st)
            _call("mrla_base_gate_fwd", 0, _ptr(mom), _ptr(wq32), _ptr(wk32), ks, _ptr(stage.K), _ptr(stage.P), _ptr(q), b, c,
                   h * w, d, T, t, st)
            _call("mrla_base_attend_fwd", nb * ((t + 1) if nhwc else (t + 2)), None if nhwc else _ptr(xc),
                  _ptr(wv32), _ptr(stage.V), _ptr(stage.P), _ptr(attn), _ptr(amom), b, c, h, w, d, T, t, dt, layout, st,
                  path=nb * (t - 1 if nhwc else t + 1))      # section 8(d): (t + 2) N per layer with the value pass + tail
            if cfg.tail:
                bn.stats(amom, None, arows, c, b * h * w // arows, st)
                _call("mrla_base_tail_fwd", nb * 3, _ptr(xc), _ptr(attn), _ptr(bnbuf[0]),
                      _ptr(bnbuf[1]), _ptr(dp32), _ptr(out), b, c, h, w, dt, layout, st, path=nb)
        stage.t = t
        if bn is not None:
            bn.finish()
        ctx.cfg, ctx.layout, ctx.ks, ctx.stage, ctx.t = cfg, layout, ks, stage, t
        ctx.shapes = (wq.shape, wk.shape, wv.shape)
        ctx.wv_stride = wv.stride()
        ctx.pdtypes = (wq.dtype, wk.dtype, wv.dtype, gamma.dtype if gamma is not None else None)
        # conv3's raw output, when the BatchNorm behind it was deferred and its backward sums can ride in the value backward
        keep_pre = (nhwc and cfg.fuse and cfg.pre_box is not None
                    and L.load().mrla_base_value_bwd_pre_sums(b, c, h, w, dt, layout) == 1)
        ctx.save_for_backward(xc, attn if cfg.tail else None, wq32, wk32, wv32, gamma32, dp32, mom, q, bnbuf,
                              pre if keep_pre else None)
        if nhwc and x.is_contiguous() and not x.is_contiguous(memory_format=_CL):
            return out.contiguous()          # an NCHW caller of an NHWC stage gets NCHW-contiguous memory back
        return out

    @staticmethod
    @_on_device
    def backward(ctx, dout):
        xc, attn, wq32, wk32, wv32, gamma32, dp32, mom, q, bnbuf, pre = ctx.saved_tensors
        cfg, layout, ks, stage, t = ctx.cfg, ctx.layout, ctx.ks, ctx.stage, ctx.t
        b, c, h, w = xc.shape
        d, T = cfg.d, stage.T
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        if dout.dtype != xc.dtype:
            dout = dout.to(xc.dtype)
        dout = _layout_of(dout, layout)[1]
        nhwc = layout == L.NHWC
        first = stage.begin_layer_backward(t)
        Tc = stage.bwd_top            # later layers that received no gradient in this pass left no dA slot behind
        es = xc.element_size()

        nb = xc.numel() * es
        kb = tmom = None
        trows = 1
        if cfg.tail:
            trows = L.load().mrla_bn_moment_rows(b, c, h, w, layout) if nhwc else b
            tmom = torch.empty((trows, c, 2), dtype=torch.float32, device=dev)
            kb = _BnBackward(c, dev)
        pmom = torch.empty((b, c, t), dtype=torch.float32, device=dev)
        ppart, prows = pmom, 0                       # (the NCHW pass leaves <dA_t, V_j> in pmom itself)
        dv = pre_tmom = center = None
        if nhwc:
            prows = L.load().mrla_base_pmom_rows(b, c, h, w, dt, layout)
            L.check(min(prows, 0), "mrla_base_pmom_rows")
            ppart = torch.empty((prows, t, c), dtype=torch.float32, device=dev)
            dv = torch.empty((b, h, w, c), dtype=xc.dtype, device=dev)      # dV_t from the dA slots t..Tc
        dyx = torch.empty((b, c), dtype=torch.float32, device=dev)
        dwqk_part = torch.empty((b, 2 * ks), dtype=torch.float32, device=dev)
        rows = L.load().mrla_light_wgrad_rows(b, c, h, w, dt, layout)
        L.check(min(rows, 0), "mrla_light_wgrad_rows")
        dwv_part = torch.empty((rows, c * 9), dtype=torch.float32, device=dev)
        dx = torch.empty_like(xc)
        res = int(cfg.tail) | (2 if cfg.fuse else 0)
        if pre is not None:
            # the deferred bn3's backward sums (sum dpre, sum dpre*(y3 - mean)) ride in the value pass: one more row fetch, no 2N pass
            pre_tmom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
            center = _ptr(cfg.pre_box.center)
        wsum = torch.empty((c * 9 + 2 * ks,), dtype=torch.float32, device=dev)
        if nhwc and _seq():     # the whole layer + tail backward: one call (mrla_base_layer_bwd)
            L.call("mrla_base_layer_bwd", _ptr(dout), _ptr(xc), _ptr(attn), _ptr(wq32), _ptr(wk32), ks, _ptr(wv32),
                   _ptr(gamma32), _ptr(dp32), _ptr(mom), _ptr(q), _ptr(bnbuf), cfg.bn_mode if cfg.tail else L.BN_NONE,
                   _ptr(stage.V), _ptr(stage.dA), _ptr(stage.K), _ptr(stage.dK), _ptr(stage.P), _ptr(tmom), trows,
                   _ptr(kb.small) if cfg.tail else None, _ptr(ppart), prows, _ptr(pmom), _ptr(dyx), _ptr(dwqk_part), _ptr(dv),
                   _ptr(dwv_part), rows, _ptr(dx), _ptr(pre), center, _ptr(pre_tmom), _ptr(wsum),
                   int(cfg.tail), int(first), res, b, c, h, w, d, T, t, Tc, dt, st)
        else:
            cb = None
            if cfg.tail:
                center_mean = bnbuf[2] if nhwc else None      # sums about the saved batch mean (the NCHW slab kernel keeps raw sums)
                _call("mrla_base_tail_stats_bwd", nb * 2, _ptr(dout), _ptr(attn), _ptr(bnbuf[0]), _ptr(bnbuf[1]),
                      _ptr(center_mean), _ptr(dp32), _ptr(tmom), b, c, h, w, dt, layout, st)
                cb = kb.stats(tmom, gamma32, bnbuf, cfg.bn_mode, int(nhwc), trows, c, b * h * w // trows, st)
            # (t + 3) N of streams + the fp32 partial rows of <dA_t, V_j> (one row of t x c floats per 16-pixel tile: 2 / 16 of the
            # V bytes it reads -- the "9 %" the PMC pass sees above (t + 3) N; mrla_base_pmom_reduce reads them back)
            _call("mrla_base_attend_bwd", nb * (t + 3) + (ppart.numel() * 4 if nhwc else 0), _ptr(dout), _ptr(attn),
                  _ptr(bnbuf[0]) if cfg.tail else None, _ptr(bnbuf[1]) if cfg.tail else None, _ptr(dp32), _ptr(cb),
                  _ptr(stage.V), _ptr(stage.dA), _ptr(ppart), b, c, h, w, T, t, dt, layout, st,
                  alg=nb * (t + 3),
                  path=nb * (t + 1))                         # section 8(d): ~(2t + 3) N per layer, backward
            if nhwc:
                _call("mrla_base_pmom_reduce", (ppart.numel() + pmom.numel()) * 4, _ptr(ppart), _ptr(pmom), b, c, t, prows, st)
            _call("mrla_base_gate_bwd", 0, _ptr(mom), _ptr(pmom), _ptr(stage.P), _ptr(q), _ptr(stage.K), _ptr(stage.dK),
                   _ptr(wq32), _ptr(wk32), ks, _ptr(dyx), _ptr(dwqk_part), b, c, h * w, d, T, t, int(first), st)
            if nhwc:                # dV_t from the dA slots t..Tc, then the transposed 3x3 pass
                _call("mrla_base_dv_combine", nb * (Tc - t + 2), _ptr(stage.dA), _ptr(stage.P), _ptr(dv),
                      b, c, h, w, d, T, t, Tc, dt, layout, st, path=nb * (Tc - t + 1))
                _call("mrla_base_value_bwd_dv", nb * (4 + (pre is not None)), _ptr(dout), _ptr(xc), _ptr(wv32),
                      _ptr(dv), _ptr(dyx), _ptr(dx), _ptr(dwv_part), _ptr(pre), center, _ptr(pre_tmom), b, c, h, w, res, dt,
                      layout, st, alg=nb * 4, path=nb)
            else:
                _call("mrla_base_value_bwd", nb * (Tc - t + 4), _ptr(dout), _ptr(xc), _ptr(wv32),
                      _ptr(stage.dA), _ptr(stage.P), _ptr(dyx), _ptr(dx), _ptr(dwv_part), b, c, h, w, d, T, t, Tc, res, dt,
                      layout, st, path=nb * (Tc - t + 2))
            _call("mrla_reduce_rows2", 0, _ptr(dwv_part), _ptr(wsum), rows, c * 9, _ptr(dwqk_part), _ptr(wsum[c * 9:]), b, 2 * ks, st)
        if pre_tmom is not None:
            cfg.pre_box.put(dx, pre_tmom, rows)
        dgamma, dbeta = kb.grads(ctx.pdtypes[3]) if cfg.tail else (None, None)
        sq, sk, sv = ctx.shapes
        tq, tk, tv, _ = ctx.pdtypes
        return (dx, dx if cfg.fuse else None, wsum[c * 9:c * 9 + ks].view(sq).to(tq), wsum[c * 9 + ks:].view(sk).to(tk),
                _grad_like(wsum[:c * 9].to(tv), sv, ctx.wv_stride), dgamma, dbeta, None, None, None, None, None)


def mrla_base(x, wq, wk, wv, d, stage, bn=None, dp=None, identity=None):
    """One MRLA-base layer on `stage` (a BaseStage).  bn: None (bare layer, returns attn) or the dict of
    mrla_light(); with bn the block tail x + dp*relu(BN(attn)) is fused in.  identity: when given, `x` is the
    bottleneck's pre-activation and x_t = relu(x + identity) is formed inside the pooling pass."""
    fuse = identity is not None
    pre_affine, pre_box = getattr(x, "_mrla_affine", None), getattr(x, "_mrla_bn_box", None)
    if pre_affine is not None and not (fuse and stage.layout == L.NHWC):
        raise L.MrlaHipError("a deferred BatchNorm output can only feed the fused producer of an NHWC MRLA-base stage")
    if bn is None:
        return _BaseFn.apply(x, identity, wq, wk, wv, None, None, None, None, None, stage,
                             BaseConfig(d, fuse=fuse, pre_affine=pre_affine, pre_box=pre_box))
    cfg = BaseConfig(d, L.BN_TRAIN if bn["training"] else L.BN_EVAL, bn.get("momentum", 0.1), bn.get("eps", 1e-5), True,
                     fuse, pre_affine, pre_box)
    return _BaseFn.apply(x, identity, wq, wk, wv, bn["weight"], bn["bias"], bn["running_mean"], bn["running_var"], dp,
                         stage, cfg)


# ======================================================================================================
# MRLA-light on token sequences (DeiT)
# ======================================================================================================
class _TokenLightFn(torch.autograd.Function):
    """out = res*x + cat(LN_x(x)[:, :1], a*gelu(dwconv3x3(LN_x(x) map)) + lam*LN_o(o_prev)[:, 1:])
    (deit_mrla_light.py:194-209 and the block residual :234)."""

    @staticmethod
    @_on_device
    def forward(ctx, x, o_prev, lnx_w, lnx_b, lno_w, lno_b, wq, wk, wv, lam, d, eps, res):
        _require_cuda(x, "mrla token forward")
        if x.dim() != 3 or o_prev.shape != x.shape or o_prev.dtype != x.dtype:
            raise L.MrlaHipError("expected x and o_prev of identical shape [b, n, c] and dtype")
        xc, oc = x.contiguous(), o_prev.contiguous()
        b, n, c = xc.shape
        side = int(round((n - 1) ** 0.5))
        if side * side != n - 1 or c % d:
            raise L.MrlaHipError(f"token count {n} is not 1 + a perfect square, or c={c} not divisible by d={d}")
        if c % 16 or c > 1024:
            # refused here, before the statistics and gate kernels of the sequence have run for nothing: the apply kernels
            # take 16-channel chunks (tokens.hip: chunk_for) and the statistics kernel holds a row of at most 64 * 16 channels
            raise L.MrlaHipError(f"mrla_token_light: c={c} is not a multiple of 16 up to 1024: "
                                 "unsupported shape/layout for the HIP kernels")
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        p32 = [_f32(t).reshape(-1) for t in (lnx_w, lnx_b, lno_w, lno_b, wq, wk, lam)]
        wxw, wxb, wow, wob, wq32, wk32, lam32 = p32
        wv32 = _f32(wv).reshape(c, 9)
        ks = wq32.numel()
        stats = torch.empty((b, n, 4), dtype=torch.float32, device=dev)
        mom = torch.empty((b, c, L.FWD_MOMENTS), dtype=torch.float32, device=dev)
        gate = torch.empty((b, c // d), dtype=torch.float32, device=dev)
        out = torch.empty_like(xc)
        if _seq():
            L.call("mrla_token_light_fwd", _ptr(xc), _ptr(oc), _ptr(wxw), _ptr(wxb), _ptr(wow), _ptr(wob), _ptr(wq32),
                   _ptr(wk32), ks, _ptr(wv32), _ptr(lam32), float(eps), _ptr(stats), _ptr(mom), _ptr(gate), _ptr(out), b, n,
                   c, d, int(res), dt, st)
        else:
            _call("mrla_token_norm_pool", 0, _ptr(xc), _ptr(oc), _ptr(wxw), _ptr(wxb), float(eps), _ptr(stats), _ptr(mom), b, n,
                   c, dt, st)
            _call("mrla_light_gate_fwd", 0, _ptr(mom), _ptr(wq32), _ptr(wk32), ks, _ptr(gate), b, c, n - 1, d, st)
            _call("mrla_token_apply_fwd", xc.numel() * xc.element_size() * 3, _ptr(xc), _ptr(oc), _ptr(stats), _ptr(wxw),
                  _ptr(wxb), _ptr(wow), _ptr(wob), _ptr(wv32), _ptr(gate), _ptr(lam32), _ptr(out), b, n, c, d, int(res), dt, st,
                  path=xc.numel() * xc.element_size() * 3)
        ctx.d, ctx.res, ctx.ks = d, int(res), ks
        ctx.meta = [(t.shape, t.dtype) for t in (lnx_w, lnx_b, lno_w, lno_b, wq, wk, wv, lam)]
        ctx.save_for_backward(xc, oc, wxw, wxb, wow, wob, wq32, wk32, wv32, lam32, stats, mom, gate)
        return out

    @staticmethod
    @_on_device
    def backward(ctx, dout):
        xc, oc, wxw, wxb, wow, wob, wq32, wk32, wv32, lam32, stats, mom, gate = ctx.saved_tensors
        b, n, c = xc.shape
        d, res, ks = ctx.d, ctx.res, ctx.ks
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        if dout.dtype != xc.dtype:
            dout = dout.to(xc.dtype)
        dout = dout.contiguous()
        es = xc.element_size()
        # one pass over the map (dxn without the pooled-descriptor term dy, bmom, the parameter partials); the gate backward
        # turns bmom into dy and completes the LayerNorm partials with it; the LayerNorm backward adds dy as it reads dxn
        bmom = torch.empty((b, c, L.BWD_MOMENTS), dtype=torch.float32, device=dev)
        dxn = torch.empty((b, n, c), dtype=torch.float32, device=dev)
        prow = L.load().mrla_token_part_rows(b, n, c, dt)
        L.check(min(prow, 0), "mrla_token_part_rows")
        part = torch.empty((prow, c * L.TOKEN_PARTIALS), dtype=torch.float32, device=dev)
        dyx = torch.empty((b, c), dtype=torch.float32, device=dev)
        dwqk_part = torch.empty((b, 2 * ks), dtype=torch.float32, device=dev)
        dx, do = torch.empty_like(xc), torch.empty_like(oc)
        sums = torch.empty((c * L.TOKEN_PARTIALS + 2 * ks,), dtype=torch.float32, device=dev)
        if _seq():
            try:
                L.call("mrla_token_light_bwd", _ptr(dout), _ptr(xc), _ptr(oc), _ptr(stats), _ptr(wxw), _ptr(wxb),
                       _ptr(wow), _ptr(wob), _ptr(wq32), _ptr(wk32), ks, _ptr(wv32), _ptr(gate), _ptr(lam32), _ptr(mom),
                       _ptr(dxn), _ptr(part), prow, _ptr(bmom), _ptr(dyx), _ptr(dwqk_part), _ptr(dx), _ptr(do), _ptr(sums),
                       b, n, c, d, res, dt, st)
            except L.MrlaHipError as e:
                if getattr(e, "code", None) != L.EUNSUPPORTED:
                    raise
                # the sequence's first pass is the only one with a shape limit of its own: two LDS tiles of the map where
                # c % 64 != 0 (side <= 30, while the forward's single tile serves side <= 46)
                err = L.MrlaHipError(f"{e}: its first pass, mrla_token_apply_bwd, does not take c={c} at a "
                                     f"{n - 1}-token map (c % 64 != 0 serves a map side of at most 30 in the backward)")
                err.code = e.code
                raise err from None
        else:
            _call("mrla_token_apply_bwd", xc.numel() * es * 3 + dxn.numel() * 4, _ptr(dout), _ptr(xc), _ptr(oc), _ptr(stats),
                  _ptr(wxw), _ptr(wxb), _ptr(wow), _ptr(wob), _ptr(wv32), _ptr(gate), _ptr(lam32), _ptr(dxn), _ptr(part),
                  _ptr(bmom), b, n, c, d, dt, st, path=xc.numel() * es * 5)      # section 8(d) backward: 5 N s for the block
            _call("mrla_token_gate_bwd", 0, _ptr(mom), _ptr(bmom), _ptr(gate), _ptr(wq32), _ptr(wk32), ks, _ptr(dyx),
                   _ptr(dwqk_part), _ptr(part), b, n, c, d, dt, st)
            _call("mrla_token_ln_bwd", xc.numel() * es * 5 + dxn.numel() * 4, _ptr(dout), _ptr(xc), _ptr(oc), _ptr(dxn),
                  _ptr(dyx), _ptr(stats), _ptr(wxw), _ptr(wow), _ptr(lam32), _ptr(dx), _ptr(do), b, n, c, res, dt, st)
            _call("mrla_reduce_rows2", 0, _ptr(part), _ptr(sums), prow, c * L.TOKEN_PARTIALS, _ptr(dwqk_part),
                   _ptr(sums[c * L.TOKEN_PARTIALS:]), b, 2 * ks, st)
        pc = sums[:c * L.TOKEN_PARTIALS].view(c, L.TOKEN_PARTIALS)
        dwqk = sums[c * L.TOKEN_PARTIALS:]
        raw = (pc[:, 10], pc[:, 11], pc[:, 12], pc[:, 13], dwqk[:ks], dwqk[ks:], pc[:, :9], pc[:, 9])
        grads = [g.reshape(shape).to(dtype) for g, (shape, dtype) in zip(raw, ctx.meta)]
        return (dx, do, *grads, None, None, None)


def mrla_token_light(x, o_prev, lnx_w, lnx_b, lno_w, lno_b, wq, wk, wv, lam, d, eps=1e-6, res=False):
    return _TokenLightFn.apply(x, o_prev, lnx_w, lnx_b, lno_w, lno_b, wq, wk, wv, lam, d, eps, res)


# ======================================================================================================
# MRLA-base on token sequences (DeiT)
# ======================================================================================================
def token_base_supported(x, d):
    """True when the fused token module of MRLA-base (LayerNorm on load, map rows written in place) takes `x` [b, n, c]."""
    if x.dim() != 3 or not x.is_cuda or x.dtype not in _DT:
        return False
    b, n, c = x.shape
    return c % d == 0 and L.load().mrla_token_base_supported(b, n, c, _DT[x.dtype]) == 1


class _TokenBaseFn(torch.autograd.Function):
    """out = cat(LN_x(x)[:, :1], mrla_base_layer(LN_x(x)[:, 1:] as a 14x14 map)) without materialising LN_x(x), the map view
    or the cat (deit/deit_mrla_base.py:224-243).  The K / V history lives in `stage` (slot-major NHWC rings)."""

    @staticmethod
    @_on_device
    def forward(ctx, x, lnx_w, lnx_b, wq, wk, wv, stage, d, eps):
        _require_cuda(x, "mrla token-base forward")
        xc = x.contiguous()
        b, n, c = xc.shape
        side = int(round((n - 1) ** 0.5))
        if (b, c, side, side, d) != (stage.b, stage.c, stage.h, stage.w, stage.d) or xc.dtype != stage.dtype \
                or stage.layout != L.NHWC:
            raise L.MrlaHipError("input does not match the stage's K/V history (shape/dtype/layout); is init_cell set on "
                                 "the first block?")
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        wxw, wxb, wq32, wk32 = (_f32(t).reshape(-1) for t in (lnx_w, lnx_b, wq, wk))
        wv32 = _f32(wv).reshape(c, 9)
        ks = wq32.numel()
        es = xc.element_size()
        stats = torch.empty((b, n, 4), dtype=torch.float32, device=dev)
        mom = torch.empty((b, c, L.FWD_MOMENTS), dtype=torch.float32, device=dev)
        _call("mrla_token_norm_pool", 0, _ptr(xc), None, _ptr(wxw), _ptr(wxb), float(eps), _ptr(stats), _ptr(mom), b, n, c,
               dt, st)
        stage.reserve_slot()
        t, T = stage.t + 1, stage.T
        _call("mrla_token_base_value_fwd", xc.numel() * es * 2, _ptr(xc), _ptr(stats), _ptr(wxw), _ptr(wxb), _ptr(wv32),
              _ptr(stage.V[t - 1]), b, n, c, dt, st, path=xc.numel() * es * 2)
        q = torch.empty((b, c), dtype=torch.float32, device=dev)
        _call("mrla_base_gate_fwd", 0, _ptr(mom), _ptr(wq32), _ptr(wk32), ks, _ptr(stage.K), _ptr(stage.P), _ptr(q), b, c,
               n - 1, d, T, t, st)
        out = torch.empty_like(xc)
        arows = L.load().mrla_base_tile_rows(b, c, side, side, dt, L.NHWC)
        L.check(min(arows, 0), "mrla_base_tile_rows")
        amom = torch.empty((arows, c, 2), dtype=torch.float32, device=dev)
        _call("mrla_token_base_attend_fwd", xc.numel() * es * (t + 1), _ptr(stage.V), _ptr(stage.P), _ptr(xc), _ptr(stats),
              _ptr(wxw), _ptr(wxb), _ptr(out), _ptr(amom), b, n, c, d, T, t, dt, st, path=xc.numel() * es * t)
        stage.t = t
        ctx.stage, ctx.t, ctx.d, ctx.ks, ctx.side = stage, t, d, ks, side
        ctx.meta = [(p.shape, p.dtype) for p in (lnx_w, lnx_b, wq, wk, wv)]
        ctx.wv_stride = wv.stride()
        ctx.save_for_backward(xc, wxw, wxb, wq32, wk32, wv32, stats, mom, q)
        return out

    @staticmethod
    @_on_device
    def backward(ctx, dout):
        xc, wxw, wxb, wq32, wk32, wv32, stats, mom, q = ctx.saved_tensors
        stage, t, d, ks, side = ctx.stage, ctx.t, ctx.d, ctx.ks, ctx.side
        b, n, c = xc.shape
        T = stage.T
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        if dout.dtype != xc.dtype:
            dout = dout.to(xc.dtype)
        dout = dout.contiguous()
        es = xc.element_size()
        first = stage.begin_layer_backward(t)
        Tc = stage.bwd_top
        pmom = torch.empty((b, c, t), dtype=torch.float32, device=dev)
        prows = L.load().mrla_base_pmom_rows(b, c, side, side, dt, L.NHWC)
        L.check(min(prows, 0), "mrla_base_pmom_rows")
        ppart = torch.empty((prows, t, c), dtype=torch.float32, device=dev)
        _call("mrla_token_base_attend_bwd", xc.numel() * es * (t + 2), _ptr(dout), _ptr(stage.V), _ptr(stage.dA), _ptr(ppart),
              b, n, c, T, t, dt, st, path=xc.numel() * es * (t + 1))
        _call("mrla_base_pmom_reduce", 0, _ptr(ppart), _ptr(pmom), b, c, t, prows, st)
        dv = torch.empty((b, side, side, c), dtype=xc.dtype, device=dev)
        _call("mrla_base_dv_combine", xc.numel() * es * (Tc - t + 2), _ptr(stage.dA), _ptr(stage.P), _ptr(dv), b, c, side,
              side, d, T, t, Tc, dt, L.NHWC, st, path=xc.numel() * es * (Tc - t + 1))
        dxn = torch.empty((b, n, c), dtype=torch.float32, device=dev)
        prow = L.load().mrla_token_part_rows(b, n, c, dt)
        L.check(min(prow, 0), "mrla_token_part_rows")
        part = torch.empty((prow, c * L.TOKEN_PARTIALS), dtype=torch.float32, device=dev)
        _call("mrla_token_base_value_bwd", xc.numel() * es * 2 + dxn.numel() * 4, _ptr(dout), _ptr(xc), _ptr(stats),
              _ptr(wxw), _ptr(wxb), _ptr(wv32), _ptr(dv), _ptr(dxn), _ptr(part), b, n, c, dt, st, path=xc.numel() * es)
        dyx = torch.empty((b, c), dtype=torch.float32, device=dev)
        dwqk_part = torch.empty((b, 2 * ks), dtype=torch.float32, device=dev)
        _call("mrla_token_base_gate_bwd", 0, _ptr(mom), _ptr(pmom), _ptr(stage.P), _ptr(q), _ptr(stage.K), _ptr(stage.dK),
               _ptr(wq32), _ptr(wk32), ks, _ptr(dyx), _ptr(dwqk_part), _ptr(part), b, n, c, d, T, t, int(first), dt, st)
        dx = torch.empty_like(xc)
        _call("mrla_token_ln_bwd", xc.numel() * es * 3 + dxn.numel() * 4, _ptr(dout), _ptr(xc), None, _ptr(dxn), _ptr(dyx),
              _ptr(stats), _ptr(wxw), None, None, _ptr(dx), None, b, n, c, 0, dt, st)
        sums = torch.empty((c * L.TOKEN_PARTIALS + 2 * ks,), dtype=torch.float32, device=dev)
        _call("mrla_reduce_rows2", 0, _ptr(part), _ptr(sums), prow, c * L.TOKEN_PARTIALS, _ptr(dwqk_part),
               _ptr(sums[c * L.TOKEN_PARTIALS:]), b, 2 * ks, st)
        pc = sums[:c * L.TOKEN_PARTIALS].view(c, L.TOKEN_PARTIALS)
        dwqk = sums[c * L.TOKEN_PARTIALS:]
        raw = (pc[:, 10], pc[:, 11], dwqk[:ks], dwqk[ks:])
        grads = [g.reshape(shape).to(dtype) for g, (shape, dtype) in zip(raw, ctx.meta)]
        sv, tv = ctx.meta[4]
        return (dx, *grads, _grad_like(pc[:, :9].to(tv), sv, ctx.wv_stride), None, None, None)


def mrla_token_base(x, lnx_w, lnx_b, wq, wk, wv, d, stage, eps=1e-6):
    return _TokenBaseFn.apply(x, lnx_w, lnx_b, wq, wk, wv, stage, d, eps)


# ======================================================================================================
# fused BatchNorm2d (+ReLU)  -- the producer-side epilogue in front of the MRLA tail
# ======================================================================================================
class _BnActState:
    """What the backward of relu?(BatchNorm2d(x)) needs beside its saved tensors (xc, gamma32, bnbuf); holds no tensor of the
    graph (`box` is the _DeferredBnBox of a deferred BatchNorm, or None)."""
    __slots__ = ("layout", "rows", "relu", "training", "gdtype", "box")

    def __init__(self, layout, rows, relu, training, gdtype, box):
        self.layout, self.rows, self.relu, self.training, self.gdtype, self.box = layout, rows, relu, training, gdtype, box


def _bn_act_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, defer, pre_moments, box):
    """y = relu?(BatchNorm2d(x)): one statistics pass + one elementwise pass.  Returns (outputs, tensors to save, state):
    y, or -- deferred -- (x as the kernels read it, detached, and bnbuf)."""
    _require_cuda(x, "fused bn/act forward")
    layout, xc = _layout_of(x)
    b, c, h, w = xc.shape
    if layout == L.NHWC and c % (16 // xc.element_size()):
        layout, xc = _layout_of(x, L.NCHW)           # the NHWC passes move 16-byte channel vectors
    dt, dev, st = _DT[xc.dtype], xc.device, _stream()
    mode = L.BN_TRAIN if training else L.BN_EVAL
    bn = _BnForward(gamma, beta, running_mean, running_var, c, mode, momentum, eps, dev, "fused bn/act forward")
    bnbuf = bn.bnbuf
    rows = L.load().mrla_bn_moment_rows(b, c, h, w, layout)           # partial-sum rows (b, or b*nsplit for NHWC)
    frows, pivot = rows, None
    records = training and pre_moments is not None
    if records:                # the producer (the 1x1 convolution GEMM) already took them: pivoted records per row
        amom, frows = pre_moments, pre_moments.shape[0]
        if tuple(amom.shape) != (frows, c, L.GEMM_MOMENTS) or amom.dtype != torch.float32:
            raise L.MrlaHipError("pre_moments must be float32 [rows, c, MRLA_GEMM_MOMENTS] records")
    else:
        amom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
        if training:           # sums about a per-channel pivot (a sample of the channel): robust for |mean| >> sigma
            pivot = torch.empty((c,), dtype=torch.float32, device=dev)
    if defer and relu:
        raise L.MrlaHipError("a deferred BatchNorm cannot carry a ReLU")
    y = None if defer else torch.empty_like(xc)
    if _seq():
        L.call("mrla_bn_fwd", _ptr(xc), _ptr(amom) if records else None, frows, None if records else _ptr(amom), _ptr(pivot),
               rows, _ptr(bn.gamma32), _ptr(bn.beta32), _ptr(bn.rs.rm), _ptr(bn.rs.rv), mode, bn.momentum, bn.eps, _ptr(bnbuf),
               int(relu), _ptr(y), b, c, h, w, dt, layout, st)
    else:
        if records:
            bn.stats_rows(amom, frows, c, st)
        else:
            if training:
                _call("mrla_bn_plane_moments", xc.numel() * xc.element_size(), _ptr(xc), _ptr(amom), _ptr(pivot), b, c, h, w,
                      dt, layout, st)
            bn.stats(amom, pivot, frows, c, b * h * w // frows, st)
        if y is not None:
            _call("mrla_bn_act_fwd", xc.numel() * xc.element_size() * 2, _ptr(xc), _ptr(bnbuf[0]), _ptr(bnbuf[1]), int(relu),
                  _ptr(y), b, c, h, w, dt, layout, st)
    bn.finish()
    state = _BnActState(layout, rows, int(relu), training, gamma.dtype, box if defer else None)
    if state.box is not None:
        state.box.center = bnbuf[2]
    return ((xc.detach(), bnbuf) if defer else y), (xc, bn.gamma32, bnbuf), state


def _bn_act_backward(saved, state, dy):
    """(dx, dgamma, dbeta) of _bn_act_forward for the gradient `dy` of its (first) output."""
    xc, gamma32, bnbuf = saved
    b, c, h, w = xc.shape
    dt, dev, st = _DT[xc.dtype], xc.device, _stream()
    if dy.dtype != xc.dtype:
        dy = dy.to(xc.dtype)
    layout, rows = state.layout, state.rows
    handed = state.box.take(dy) if state.box is not None else None      # (sum dz, sum dz*x) taken by the producer of dy
    dy = _layout_of(dy, layout)[1]
    es = xc.element_size()
    if handed is not None:
        tmom, rows = handed
    else:
        tmom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
    kb = _BnBackward(c, dev)
    dx = torch.empty_like(xc)
    mode = L.BN_TRAIN if state.training else L.BN_EVAL
    if _seq():
        L.call("mrla_bn_bwd", _ptr(dy), _ptr(xc), _ptr(gamma32), _ptr(bnbuf), _ptr(tmom), rows, int(handed is not None), mode,
               state.relu, _ptr(kb.small), _ptr(dx), b, c, h, w, dt, layout, st)
    else:
        if handed is None:
            _call("mrla_bn_plane_dmoments", xc.numel() * es * 2, _ptr(dy), _ptr(xc), _ptr(bnbuf[0]), _ptr(bnbuf[1]),
                  _ptr(bnbuf[2]), state.relu, _ptr(tmom), b, c, h, w, dt, layout, st)
        cb = kb.stats(tmom, gamma32, bnbuf, mode, 1, rows, c, b * h * w // rows, st)
        _call("mrla_bn_act_bwd", xc.numel() * es * 3, _ptr(dy), _ptr(xc), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(cb), state.relu,
              _ptr(dx), b, c, h, w, dt, layout, st)
    return (dx,) + kb.grads(state.gdtype)


class _BnActFn(torch.autograd.Function):
    """y = relu?(BatchNorm2d(x)): one statistics pass + one elementwise pass per direction (_bn_act_forward / _backward).
    defer: skip the forward elementwise pass; the result aliases x and (scale, shift) are returned beside it for the
    consumer (the fused MRLA producer) to apply.  The backward is the same either way."""

    @staticmethod
    @_on_device
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, defer=False,
                pre_moments=None, box=None):
        ctx.set_materialize_grads(False)       # (no zero-filled gradient tensor for the non-differentiable second output)
        out, saved, ctx.state = _bn_act_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, defer,
                                                pre_moments, box)
        ctx.save_for_backward(*saved)
        if defer:
            ctx.mark_non_differentiable(out[1])
        return out

    @staticmethod
    @_on_device
    def backward(ctx, dy, _dbuf=None):
        if dy is None:
            return (None,) * 12
        return _bn_act_backward(ctx.saved_tensors, ctx.state, dy) + (None,) * 9


def bn_act(x, bn, relu, defer=False, pre_moments=None):
    """relu?(bn(x)) for an nn.BatchNorm2d module `bn` on the fused HIP passes; any other norm layer (or a layout /
    device the kernels do not handle) runs as the caller's module followed by torch.relu.
    defer=True (relu must be False): only the statistics are taken; the returned tensor aliases x and carries the
    per-channel affine as `._mrla_affine` for `mrla_light(..., pre_activation=True)` to apply in its first pass."""
    if (_is_fused_bn(bn) and x.is_cuda and x.dim() == 4
            and x.dtype in _DT and (x.is_contiguous() or x.is_contiguous(memory_format=_CL))):
        training, momentum = _bn_step(bn)
        if defer:
            box = _DeferredBnBox()
            y, buf = _BnActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum,
                                    bn.eps, False, True, pre_moments, box)
            y._mrla_affine = (buf[0], buf[1])
            y._mrla_bn_box = box
            return y
        return _BnActFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps,
                              relu, False, pre_moments)
    y = bn(x)
    return torch.relu(y) if relu else y


# ======================================================================================================
# BatchNorm2d + channel attention (SE / ECA) -- resnet_mrla_light.py:77-81,105-108
# ======================================================================================================
class _BnGateFn(torch.autograd.Function):
    """out = g * BatchNorm2d(y), g[b,c] = ECA or SE gate of the BatchNorm output's plane means ("Channel
    attention").  kind 0: ECA, weights (w [1,1,k],); kind 1: SE, weights (W1 [c/r, c], W2 [c, c/r]), its two small
    products as fp32 torch.mm on the [b,c] rows.  Everything that touches the activation is HIP: plane moments + apply
    forward (3 passes), plane dmoments + apply backward (5 passes)."""

    @staticmethod
    @_on_device
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, momentum, eps, kind, *weights):
        _require_cuda(y, "bn + channel gate forward")
        b, c, h, w = y.shape
        hw = h * w
        dt, dev, st = _DT[y.dtype], y.device, _stream()
        lay = L.NHWC
        bn = _BnForward(gamma, beta, running_mean, running_var, c, L.BN_TRAIN if training else L.BN_EVAL, momentum, eps, dev,
                        "bn + channel gate forward")
        bnbuf = bn.bnbuf
        f32 = dict(dtype=torch.float32, device=dev)
        rows = L.load().mrla_bn_moment_rows(b, c, h, w, lay)
        amom = torch.empty((rows, c, 2), **f32)
        pivot = torch.empty((c,), **f32) if training else None
        sp = torch.empty((2, b, c), **f32)                                   # S | pooled
        es = y.element_size()
        # the plane sums are wanted in eval mode too: they are the pool
        _call("mrla_bn_plane_moments", y.numel() * es, _ptr(y), _ptr(amom), _ptr(pivot), b, c, h, w, dt, lay, st)
        bn.stats(amom, pivot, rows, c, b * hw // rows, st)
        _call("mrla_bn_gate_pool", 0, _ptr(amom), _ptr(pivot), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(sp[0]), _ptr(sp[1]),
              b, c, h, w, lay, st)
        hid = None
        if kind == 0:
            wk = _f32(weights[0]).reshape(-1)
            g = torch.empty((b, c), **f32)
            _call("mrla_eca_gate_fwd", 0, _ptr(sp[1]), _ptr(wk), wk.numel(), _ptr(g), b, c, st)
            saved_w = (wk,)
        else:
            w1, w2 = _f32(weights[0]), _f32(weights[1])
            with torch.autocast("cuda", enabled=False):                      # (fp32 rows stay fp32 under autocast)
                hid = torch.relu_(torch.mm(sp[1], w1.t()))                   # [b, c/r]
                g = torch.sigmoid_(torch.mm(hid, w2.t()))
            saved_w = (w1, w2, hid)
        out = torch.empty_like(y)
        _call("mrla_bn_gate_fwd", y.numel() * es * 2, _ptr(y), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(g), _ptr(out), b, c, h, w,
              dt, lay, st)
        bn.finish()
        ctx.training, ctx.kind, ctx.rows = training, kind, rows
        ctx.gdtype, ctx.wmeta = gamma.dtype, [(t.dtype, tuple(t.shape)) for t in weights]
        ctx.save_for_backward(y, bn.gamma32, bnbuf, sp, g, *saved_w)
        return out

    @staticmethod
    @_on_device
    def backward(ctx, do):
        y, gamma32, bnbuf, sp, g, *saved_w = ctx.saved_tensors
        b, c, h, w = y.shape
        hw = h * w
        dt, dev, st = _DT[y.dtype], y.device, _stream()
        lay = L.NHWC
        if do.dtype != y.dtype:
            do = do.to(y.dtype)
        do = _layout_of(do, lay)[1]
        if do.data_ptr() % 16:                 # (a view at an odd storage offset: the passes move 16-byte vectors)
            do = do.clone(memory_format=_CL)
        f32 = dict(dtype=torch.float32, device=dev)
        es = y.element_size()
        arows = torch.empty((ctx.rows, c, 2), **f32)
        dg = torch.empty((b, c), **f32)
        tmom = torch.empty((b, c, 2), **f32)
        kb = _BnBackward(c, dev)
        sums = (_ptr(arows), _ptr(sp[0]), _ptr(g))
        bn3 = (_ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(bnbuf[2]))
        _call("mrla_bn_plane_dmoments", y.numel() * es * 2, _ptr(do), _ptr(y), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(bnbuf[2]), 0,
              _ptr(arows), b, c, h, w, dt, lay, st)
        _call("mrla_bn_gate_sums_bwd", 0, *sums, None, *bn3, _ptr(dg), None, b, c, h, w, lay, st)
        if ctx.kind == 0:
            wk = saved_w[0]
            k = wk.numel()
            q = torch.empty((b, c), **f32)
            dwp = torch.empty((b + 1, k), **f32)                             # per-image partials | their sum
            _call("mrla_eca_gate_bwd", 0, _ptr(dg), _ptr(g), _ptr(sp[1]), _ptr(wk), k, _ptr(q), _ptr(dwp), _ptr(dwp[b]), b, c,
                  hw, st)
            wgrads = (dwp[b],)
        else:
            w1, w2, hid = saved_w
            with torch.autocast("cuda", enabled=False):
                da = dg.mul_(g).mul_(1.0 - g)                                # through the sigmoid
                dw2 = torch.mm(da.t(), hid)
                dh = torch.mm(da, w2).mul_(hid > 0)
                dw1 = torch.mm(dh.t(), sp[1])
                q = torch.mm(dh, w1).div_(float(hw))
            wgrads = (dw1, dw2)
        _call("mrla_bn_gate_sums_bwd", 0, *sums, _ptr(q), *bn3, None, _ptr(tmom), b, c, h, w, lay, st)
        cb = kb.stats(tmom, gamma32, bnbuf, L.BN_TRAIN if ctx.training else L.BN_EVAL, 1, b, c, hw, st)
        dy = torch.empty_like(y)
        _call("mrla_bn_gate_bwd", y.numel() * es * 3, _ptr(do), _ptr(y), _ptr(cb), _ptr(g), _ptr(q), _ptr(dy), b, c, h, w, dt,
              lay, st)
        wg = tuple(t.reshape(shape).to(dtype) for t, (dtype, shape) in zip(wgrads, ctx.wmeta))
        return (dy,) + kb.grads(ctx.gdtype) + (None,) * 6 + wg


def bn_gate_applies(shape, dtype, channels_last, is_cuda, bn, se=None, eca=None):
    """True when se?/eca?(bn(y)) for a `y` of that shape, dtype and layout is the one HIP node _BnGateFn: the switch is on,
    no KernelTimer is active, `bn` is an nn.BatchNorm2d with affine and tracked statistics, exactly one of se / eca is given,
    and y is a channels_last CUDA tensor of a shape mrla_bn_gate_supported takes."""
    if not (CHANNEL_GATE and TIMER is None and (se is None) != (eca is None)):
        return False
    if not _is_fused_bn(bn):
        return False
    if not (is_cuda and len(shape) == 4 and dtype in _DT and channels_last):
        return False
    b, c, h, w = shape
    if min(b, c, h, w) <= 0:
        return False
    return L.load().mrla_bn_gate_supported(b, c, h, w, _DT[dtype], L.NHWC) == 1


def bn_gate(x, bn, se=None, eca=None, pre_moments=None):
    """eca?(se?(bn(x))) -- `out = self.bn3(out)`, `out = self.se(out)`, `out = self.eca(out)` of resnet_mrla_light.py:102-108
    -- for the raw output `x` of the convolution in front.  On the HIP node (bn_gate_applies) neither bn's output nor
    anything else of x's size is stored between the passes; everything else is bn_act(x, bn) followed by the eager modules
    (`pre_moments`: the producer's moment records, which only that route reads -- the HIP node takes the plane sums, which
    are its pool as well)."""
    if x.dim() == 4 and bn_gate_applies(tuple(x.shape), x.dtype, x.is_contiguous(memory_format=_CL), x.is_cuda, bn, se, eca) \
            and x.data_ptr() % 16 == 0:
        training, momentum = _bn_step(bn)
        if eca is not None:
            kind, weights = 0, (eca.conv.weight,)
        else:
            kind, weights = 1, (se.fc[0].weight, se.fc[2].weight)
        return _BnGateFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps,
                               kind, *weights)
    out = bn_act(x, bn, False, pre_moments=pre_moments)
    if se is not None:
        out = se(out)
    if eca is not None:
        out = eca(out)
    return out


class _BnReluPoolFn(torch.autograd.Function):
    """maxpool3x3/s2/p1(relu(BatchNorm2d(x))) on a channels_last tensor without the full-size intermediate
    (mrla_bn_relu_pool_*; resnet_mrla_light.py:220-222).  The statistics pass and the running-stat update are
    _BnActFn's; the window maximum follows ATen's first-maximum rule on the rounded values."""

    @staticmethod
    @_on_device
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps):
        _require_cuda(x, "fused bn/relu/maxpool forward")
        layout, xc = _layout_of(x, L.NHWC)
        b, c, h, w = xc.shape
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        mode = L.BN_TRAIN if training else L.BN_EVAL
        bn = _BnForward(gamma, beta, running_mean, running_var, c, mode, momentum, eps, dev, "fused bn/relu/maxpool forward")
        bnbuf = bn.bnbuf
        rows = L.load().mrla_bn_moment_rows(b, c, h, w, layout)
        amom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
        pivot = torch.empty((c,), dtype=torch.float32, device=dev) if training else None
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out = torch.empty((b, c, ho, wo), dtype=xc.dtype, device=dev, memory_format=_CL)
        if _seq():
            L.call("mrla_stem_fwd", _ptr(xc), _ptr(amom), _ptr(pivot), rows, _ptr(bn.gamma32), _ptr(bn.beta32), _ptr(bn.rs.rm),
                   _ptr(bn.rs.rv), mode, bn.momentum, bn.eps, _ptr(bnbuf), _ptr(out), b, c, h, w, dt, layout, st)
        else:
            if training:
                _call("mrla_bn_plane_moments", xc.numel() * xc.element_size(), _ptr(xc), _ptr(amom), _ptr(pivot), b, c, h, w, dt,
                      layout, st)
            bn.stats(amom, pivot, rows, c, b * h * w // rows, st)
            _call("mrla_bn_relu_pool_fwd", (xc.numel() + out.numel()) * xc.element_size(), _ptr(xc), _ptr(bnbuf[0]),
                  _ptr(bnbuf[1]), _ptr(out), b, c, h, w, dt, layout, st)
        bn.finish()
        ctx.training, ctx.gdtype = training, gamma.dtype
        ctx.save_for_backward(xc, bn.gamma32, bnbuf)
        return out

    @staticmethod
    @_on_device
    def backward(ctx, dp):
        xc, gamma32, bnbuf = ctx.saved_tensors
        b, c, h, w = xc.shape
        dt, dev, st = _DT[xc.dtype], xc.device, _stream()
        if dp.dtype != xc.dtype:
            dp = dp.to(xc.dtype)
        dp = _layout_of(dp, L.NHWC)[1]
        es = xc.element_size()
        rows = L.load().mrla_bn_pool_rows(b, c, h, w, dt, L.NHWC)
        L.check(min(rows, 0), "mrla_bn_pool_rows")
        tmom = torch.empty((rows, c, 2), dtype=torch.float32, device=dev)
        kb = _BnBackward(c, dev)
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        mode = L.BN_TRAIN if ctx.training else L.BN_EVAL
        if _seq():
            L.call("mrla_stem_bwd", _ptr(dp), _ptr(xc), _ptr(gamma32), _ptr(bnbuf), _ptr(tmom), rows, mode, _ptr(kb.small),
                   _ptr(dx), b, c, h, w, dt, L.NHWC, st)
        else:
            _call("mrla_bn_relu_pool_dmoments", (xc.numel() + dp.numel()) * es, _ptr(dp), _ptr(xc), _ptr(bnbuf[0]), _ptr(bnbuf[1]),
                  _ptr(bnbuf[2]), _ptr(tmom), b, c, h, w, dt, L.NHWC, st)
            cb = kb.stats(tmom, gamma32, bnbuf, mode, 1, rows, c, b * h * w // rows, st)
            if dx is not None:
                _call("mrla_bn_relu_pool_bwd", (2 * xc.numel() + dp.numel()) * es, _ptr(dp), _ptr(xc), _ptr(bnbuf[0]),
                      _ptr(bnbuf[1]), _ptr(cb), _ptr(dx), b, c, h, w, dt, L.NHWC, st)
        return (dx,) + kb.grads(ctx.gdtype) + (None,) * 5


def bn_relu_maxpool(x, bn, pool):
    """pool(relu(bn(x))) for the ResNet stem (nn.BatchNorm2d, then nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
    resnet_mrla_light.py:220-222): one fused pass per direction when x is a channels_last CUDA tensor with c % 64 == 0;
    any other configuration runs `pool(bn_act(x, bn, relu=True))`."""
    def _pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if (_is_fused_bn(bn) and type(pool) is torch.nn.MaxPool2d
            and _pair(pool.kernel_size) == (3, 3) and _pair(pool.stride) == (2, 2) and _pair(pool.padding) == (1, 1)
            and _pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices
            and x.is_cuda and x.dim() == 4 and x.dtype in _DT and x.is_contiguous(memory_format=_CL)
            and x.data_ptr() % 16 == 0
            and L.load().mrla_bn_pool_rows(x.shape[0], x.shape[1], x.shape[2], x.shape[3], _DT[x.dtype], L.NHWC) > 0):
        training, momentum = _bn_step(bn)
        return _BnReluPoolFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps)
    return pool(bn_act(x, bn, relu=True))


# ======================================================================================================
# 1x1 stride-1 convolution as an MFMA GEMM with the BatchNorm statistics in its epilogue
# ======================================================================================================
class WeightBank:
    """16-bit working copies [n, k] (and transposes [k, n]) of a model's fp32 1x1-convolution weights, refreshed by ONE
    launch of mrla_weight_bank_refresh_dt per training step: what torch.autocast does with one cast kernel per convolution
    and forward, and what the input-gradient GEMM needed one transposing copy per call for.  Built lazily for the
    eligible convolutions of a model (1x1, stride 1, no bias, fp32 weight, both channel counts multiples of 64);
    `refresh()` re-launches whenever gradients are enabled (a training forward: the optimizer will have moved the masters,
    and one launch costs 0.02 ms), whenever a HIP graph is being captured, and ALWAYS once a refresh has been captured:
    replays of that graph update the masters without touching any Python-side version counter, so after them the
    counters prove nothing.  Only a grad-free forward outside any capture history (validation loops) skips the launch
    while every weight's version counter stands still; writes the counters cannot see (`p.data.copy_(...)`) need
    `invalidate()`.
    The copies are of ONE dtype at a time, the one the bank was last refreshed for: bf16 unless refresh() is told otherwise
    or runs under fp16 CUDA autocast.  A change of dtype rebuilds the copies and the table like a first use (not
    capturable); get() hands copies out only to a caller that asks for the dtype they are of, so a bf16 bank never
    reaches an fp16 GEMM."""

    def __init__(self, convs):
        self.convs = [c for c in convs if self.eligible(c)]
        self.key = self.sig = None
        self.dtype = torch.bfloat16
        self.captured = False          # sticky: a refresh is part of some HIP graph
        self.entries = {}

    def invalidate(self):
        """Force the next refresh() to re-cast (after weight updates that bypass the version counters)."""
        self.key = None

    @staticmethod
    def eligible(conv):
        # (strided 1x1 convolutions -- the downsample branch of a stage's first block -- run the same GEMM on the
        # subsampled input: conv_bn_act)
        return (type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1)
                and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
                and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0)

    def _build(self, live, dtype):
        dev = live[0].weight.device
        total = sum(c.weight.numel() for c in live)
        self.dtype = dtype
        self.flat = torch.empty((2, total), dtype=dtype, device=dev)
        rows, off, self.entries, self.max_tiles = [], 0, {}, 1
        for c in live:
            n, k = c.out_channels, c.in_channels
            w16, w16t = self.flat[0, off:off + n * k].view(n, k), self.flat[1, off:off + n * k].view(k, n)
            rows.append([c.weight.data_ptr(), w16.data_ptr(), w16t.data_ptr(), (n << 32) | k])
            self.entries[id(c)] = (w16, w16t)
            self.max_tiles = max(self.max_tiles, (n // 64) * (k // 64))
            off += n * k
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.n = len(rows)

    def refresh(self, dtype=None):
        """dtype: torch.bfloat16 or torch.float16; None: the CUDA autocast dtype when autocast is on and is one of the two,
        else bf16."""
        if dtype is None:
            dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.bfloat16
            if dtype not in (torch.bfloat16, torch.float16):
                dtype = torch.bfloat16
        elif dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"WeightBank.refresh: dtype must be torch.bfloat16 or torch.float16, got {dtype}")
        live = [c for c in self.convs if c.weight.is_cuda and c.weight.dtype == torch.float32
                and (c.weight.is_contiguous() or c.weight.is_contiguous(memory_format=_CL))]
        if not live:
            self.entries = {}
            return self
        sig = (dtype,) + tuple((id(c), c.weight.data_ptr()) for c in live)
        capturing = torch.cuda.is_current_stream_capturing()
        if sig != self.sig:        # first use, the parameters moved (.to(), load with assign=...), or another dtype is asked for
            if capturing:                         # (the table is built with a host-to-device copy: not capturable)
                raise L.MrlaHipError("WeightBank: first use (or moved parameters, or a change of dtype) inside a HIP graph "
                                     "capture; run one forward of the model eagerly before capturing it (in the precision of the capture)")
            self._build(live, dtype)
            self.sig, self.key = sig, None
        key = tuple(c.weight._version for c in live)
        self.captured = self.captured or capturing
        if key != self.key or self.captured or torch.is_grad_enabled():
            with torch.cuda.device(self.table.device):
                L.call("mrla_weight_bank_refresh_dt", _ptr(self.table), self.n, self.max_tiles, _DT[self.dtype], _stream())
            self.key = key
        return self

    def get(self, conv, dtype=torch.bfloat16):
        """(w [n, k], w^T [k, n]) of `conv` in `dtype`, or None when it is not in the bank or the bank's copies are of
        another dtype."""
        return self.entries.get(id(conv)) if dtype == self.dtype else None


class Conv3x3Bank:
    """16-bit working copies of a model's fp32 3x3-convolution weights whose stride-1 input gradient runs as a forward
    convolution (CONV3X3_DGRAD_FLIP): per weight [n, c, 3, 3] the channels_last copy `w16` the forward multiplies with and
    `wflip`, a channels_last [c, n, 3, 3] with wflip[c, n, kh, kw] = w16[n, c, 2 - kh, 2 - kw], the operand of
    dX = conv(dY, wflip) -- all of them written by ONE launch of mrla_conv3x3_weight_bank_refresh per forward: what
    torch.autocast does with one cast kernel per convolution and forward, and what the permutation costs two elementwise
    kernels per input gradient for.
    Built lazily: a convolution becomes a member when conv3x3 first routes it (get()), so a model none of whose shapes is
    routed never calls the entry point.  A first build, a new member, moved parameters or another dtype rebuild the table
    with a host-to-device copy: not capturable -- run one forward eagerly before capturing, as for the WeightBank.
    get() refreshes at most once per bookkeeping scope (once per forward), under WeightBank.refresh's conditions: whenever
    gradients are enabled, whenever a HIP graph is being captured, and ALWAYS once a refresh has been captured (replays
    move the masters without touching a version counter); `invalidate()` after writes the counters cannot see."""

    def __init__(self):
        self.members, self.entries = [], {}          # convolutions in the order they were first routed; id -> (w16, wflip)
        self.sig = self.key = self.table = None
        self.dtype = torch.bfloat16
        self.captured = False          # sticky: a refresh is part of some HIP graph
        self.max_tiles = 1
        self._tables = []              # tables a captured refresh may still read

    def invalidate(self):
        """Force the next refresh to re-cast (after weight updates that bypass the version counters)."""
        self.key = None

    @staticmethod
    def eligible(conv):
        if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
                and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"
                and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0):
            return False
        w = conv.weight
        return (w.is_cuda and w.dtype == torch.float32 and w.data_ptr() % 16 == 0
                and (w.is_contiguous() or w.is_contiguous(memory_format=_CL)))

    def _signature(self, dtype):
        return (dtype,) + tuple((id(c), c.weight.data_ptr(), c.weight.is_contiguous()) for c in self.members)

    def _build(self, dtype, what):
        if torch.cuda.is_current_stream_capturing():      # (the table is built with a host-to-device copy: not capturable)
            raise L.MrlaHipError(f"Conv3x3Bank: {what} inside a HIP graph capture; run one forward of the model eagerly before "
                                 "capturing it (in the precision of the capture)")
        self.members = [c for c in self.members if self.eligible(c)]
        if dtype != self.dtype:
            self.entries = {}
        self.dtype, rows, entries, self.max_tiles = dtype, [], {}, 1
        for c in self.members:
            w, n, k = c.weight, c.out_channels, c.in_channels
            held = self.entries.get(id(c))
            if held is None or held[0].device != w.device:
                held = (torch.empty((n, k, 3, 3), dtype=dtype, device=w.device, memory_format=_CL),
                        torch.empty((k, n, 3, 3), dtype=dtype, device=w.device, memory_format=_CL))
            entries[id(c)] = held
            rows.append([w.data_ptr(), held[0].data_ptr(), held[1].data_ptr(), (n << 32) | k, 0 if w.is_contiguous() else 1])
            self.max_tiles = max(self.max_tiles, 9 * (n // 64) * (k // 64))
        self.entries = entries
        if self.captured and self.table is not None:
            self._tables.append(self.table)
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.members[0].weight.device) if rows else None
        self.sig, self.key = self._signature(dtype), None

    def _refresh(self, dtype):
        if self._signature(dtype) != self.sig or not all(self.eligible(c) for c in self.members):
            self._build(dtype, "moved parameters or a change of dtype")
        if self.table is None:
            return
        key = tuple(c.weight._version for c in self.members)
        self.captured = self.captured or torch.cuda.is_current_stream_capturing()
        if key != self.key or self.captured or torch.is_grad_enabled():
            with torch.cuda.device(self.table.device):
                L.call("mrla_conv3x3_weight_bank_refresh", _ptr(self.table), len(self.members), self.max_tiles,
                       _DT[self.dtype], _stream())
            self.key = key

    def get(self, conv, dtype, book):
        """(w16, wflip) of `conv` in `dtype` (torch.bfloat16 or torch.float16), as of this forward -- `book`: its bookkeeping
        scope, which remembers that the refresh ran -- or None for a convolution the bank does not take."""
        if dtype not in (torch.bfloat16, torch.float16) or not self.eligible(conv):
            return None
        if id(conv) not in self.entries or dtype != self.dtype:
            if not any(c is conv for c in self.members):
                self.members.append(conv)
            try:
                self._build(dtype, "first use of a convolution (or a change of dtype)")
            except L.MrlaHipError:
                self.members = [c for c in self.members if id(c) in self.entries]
                raise
            book.bank3_fresh = False
        if not book.bank3_fresh:
            self._refresh(dtype)
            book.bank3_fresh = True
        return self.entries.get(id(conv))


class _GemmState:
    """What the backward of the 1x1 GEMM convolution needs beside its saved tensors (x, w, w16t); holds no tensor."""
    __slots__ = ("sub", "wshape", "wstride", "wdtype", "f32")

    def __init__(self, sub, wshape, wstride, wdtype, f32):
        self.sub, self.wshape, self.wstride, self.wdtype, self.f32 = sub, wshape, wstride, wdtype, f32


def _conv1x1_forward(x, w, want_moments, passthrough, w16, w16t, sub):
    """The forward of _Conv1x1Fn (its docstrings describe the arguments).  Returns (outputs, tensors to save, state):
    outputs = (y, moment records or an empty tensor[, x or its subsample])."""
    sub = tuple(sub) if (passthrough and sub is not None) else None
    b, k, h, wd = x.shape
    n = w.shape[0]
    m = b * h * wd
    dev, st = x.device, _stream()
    wshape, wstride, wdtype = w.shape, w.stride(), w.dtype   # [n, k] or the module's [n, k, 1, 1]
    if w16 is not None:
        w = w16
    else:
        w = w.reshape(n, k)                            # (a view: the 1x1 taps carry no data)
        if not w.is_contiguous():
            w = w.contiguous()
    part = None
    # fp32 operands (CONV1X1_F32): the GEMMs of conv1x1_f32.hip; remembered for the backward, whatever the switch says then
    f32 = (CONV1X1_F32 and x.dtype == torch.float32 and w.dtype == torch.float32 and x.data_ptr() % 16 == 0
           and w.data_ptr() % 16 == 0)
    rows = (L.load().mrla_conv1x1_f32_rows(m, k, n) if f32
            else L.load().mrla_conv1x1_rows(m, k, n, _DT[x.dtype]))   # > 0: supported, that many moment-record rows; < 0: not taken
    if f32 and rows > 0:
        y = torch.empty((b, n, h, wd), dtype=x.dtype, device=dev, memory_format=_CL)
        if want_moments:
            part = torch.empty((rows, n, L.GEMM_MOMENTS), dtype=torch.float32, device=dev)
        _call("mrla_conv1x1_f32_fwd", (x.numel() + y.numel()) * 4, _ptr(x), _ptr(w), 0, _ptr(y), _ptr(part), m, k, n, st)
    elif rows >= 0:
        y = torch.empty((b, n, h, wd), dtype=x.dtype, device=dev, memory_format=_CL)
        if want_moments and rows > 0:
            part = torch.empty((rows, n, L.GEMM_MOMENTS), dtype=torch.float32, device=dev)
        _call("mrla_conv1x1_fwd", (x.numel() + y.numel()) * x.element_size(), _ptr(x), _ptr(w), _ptr(y), _ptr(part), m, k,
              n, _DT[x.dtype], st)
    else:
        y = torch.nn.functional.conv2d(x, w.view(n, k, 1, 1))
    if part is None:
        part = torch.empty(0, device=dev)
    outs = (y, part)
    if sub is not None:
        outs += (x[:, :, ::sub[0], ::sub[1]].contiguous(memory_format=_CL),)
    elif passthrough:           # x itself as a third output: its gradient (the shortcut's) comes back to the backward
        outs += (x,)
    return outs, (x, w, w16t), _GemmState(sub, wshape, wstride, wdtype, f32)


def _conv1x1_backward(saved, state, needs, dy, d_through):
    """(gx, gw) of _conv1x1_forward.  needs: (the input, the weight) want their gradient; dy: the gradient of y, None when
    only the shortcut carried one; d_through: the gradient of the third output, or None."""
    x, w, w16t = saved
    sub = state.sub
    sh, sw = sub if sub is not None else (1, 1)
    if dy is None:             # only the shortcut carried a gradient
        if d_through is not None and sub is not None:
            d_through = _scatter_subsample(d_through, x.shape, sh, sw, _CL)
        return (d_through if needs[0] else None), None
    dy = dy.contiguous(memory_format=_CL)
    n, k = w.shape
    b, _, h, wd = x.shape
    m = b * h * wd
    lib, dt = L.load(), _DT[x.dtype]
    need_x, need_w = needs
    gx = gw = None
    same = dy.dtype == x.dtype and dy.data_ptr() % 16 == 0
    # the input gradient is the same GEMM with the transposed weight: dX[m, k] = sum_n dY[m, n] * W^T[k, n]
    # (no memset of dX, as MIOpen's backward-data solver needs); shapes the kernel does not take stay on MIOpen
    if d_through is not None and (d_through.dtype != x.dtype or not d_through.is_contiguous(memory_format=_CL)
                                  or d_through.data_ptr() % 16):
        d_through = d_through.to(x.dtype).contiguous(memory_format=_CL)
    if state.f32:
        # fp32: dX on the weight as stored ([n, k] is reduction-major for this product: w_trans = 1, no transposed copy),
        # dW straight into an fp32 [n, k]; the shortcut's gradient is added by the tail below
        if need_x and same and lib.mrla_conv1x1_f32_rows(m, n, k) > 0:
            gx = torch.empty_like(x)
            _call("mrla_conv1x1_f32_bwd_data", (dy.numel() + gx.numel()) * 4, _ptr(dy), _ptr(w), 1, _ptr(gx), None, m, n, k,
                  _stream(), entry="mrla_conv1x1_f32_fwd")
            need_x = False
        rows = lib.mrla_conv1x1_f32_wgrad_rows(m, k, n) if (need_w and same) else 0
        if rows > 0:
            part = torch.empty((rows, n, k), dtype=torch.float32, device=x.device)
            gw = torch.empty((n, k), dtype=torch.float32, device=x.device)
            _call("mrla_conv1x1_f32_wgrad", (dy.numel() + x.numel()) * 4, _ptr(dy), _ptr(x), _ptr(part), _ptr(gw), m, k, n,
                  _stream())
            need_w = False
    elif need_x and same and lib.mrla_conv1x1_rows(m, n, k, dt) >= 0:
        gx = torch.empty_like(x)
        wt = w16t if w16t is not None else w.t().contiguous()
        if d_through is not None and SHORTCUT_ADDEND and lib.mrla_conv1x1_addend_supported(m, n, k, sh, sw, dt) == 1:
            # ... + the shortcut's gradient inside the GEMM, whichever kernel form takes the shape, and from the compact
            # gradient of a strided block's subsample as it is (no zero-fill, no scatter, a quarter of the addend bytes)
            _call("mrla_conv1x1_bwd_data", (dy.numel() + gx.numel() + d_through.numel()) * x.element_size(), _ptr(dy),
                  _ptr(wt), _ptr(d_through), _ptr(gx), m, n, k, b, h, wd, sh, sw, dt, _stream(),
                  entry="mrla_conv1x1_fwd_addend")
            d_through = None
        elif d_through is not None and lib.mrla_conv1x1_add_supported(m, n, k, dt) == 1:
            # ... + the shortcut's gradient in the wide GEMM's epilogue (fp32 sum, one rounding) instead of a separate
            # accumulation pass over the block input's gradient
            if sub is not None:
                d_through, sub = _scatter_subsample(d_through, x.shape, sh, sw, _CL), None
            _call("mrla_conv1x1_bwd_data", (dy.numel() + 2 * gx.numel()) * x.element_size(), _ptr(dy), _ptr(wt),
                  _ptr(d_through), _ptr(gx), m, n, k, dt, _stream(), entry="mrla_conv1x1_fwd_add")
            d_through = None
        else:
            _call("mrla_conv1x1_bwd_data", (dy.numel() + gx.numel()) * x.element_size(), _ptr(dy), _ptr(wt), _ptr(gx),
                  None, m, n, k, dt, _stream(), entry="mrla_conv1x1_fwd")
        need_x = False
    # the weight gradient dW[n, k] = sum_m dY[m, n] * X[m, k]: one pass over both activations, per-workgroup partial
    # tiles summed by a second kernel (MIOpen: memset + atomics into fp32 + a cast kernel)
    if need_w and same and not state.f32 and w.dtype == x.dtype and state.wdtype in (x.dtype, torch.float32):
        rows = lib.mrla_conv1x1_wgrad_rows(m, k, n, dt)
        if rows > 0:
            part = torch.empty((rows, n, k), dtype=torch.float32, device=x.device)
            gw = torch.empty((n, k), dtype=state.wdtype, device=x.device)       # the master's dtype, no cast kernel behind
            _call("mrla_conv1x1_wgrad", (dy.numel() + x.numel()) * x.element_size(), _ptr(dy), _ptr(x), _ptr(part),
                  _ptr(gw), m, k, n, dt, _DT[state.wdtype], _stream())
            need_w = False
    if need_x or need_w:
        gx2, gw2, _ = torch.ops.aten.convolution_backward(dy, x, w.view(n, k, 1, 1), None, (1, 1), (0, 0), (1, 1), False,
                                                          (0, 0), 1, [need_x, need_w, False])
        gx = gx2 if need_x else gx
        gw = gw2.reshape(n, k) if need_w else gw
    if d_through is not None and needs[0]:
        # what no GEMM took: a shape or dtype off the HIP path, SHORTCUT_ADDEND off and a form other than the wide one
        if sub is not None:
            d_through = _scatter_subsample(d_through, x.shape, sh, sw, _CL)
        gx = gx + d_through
    if gw is not None:          # the weight's own dtype, shape AND strides (autograd's / DDP's gradient layout contract)
        gw = _grad_like(gw.to(state.wdtype), state.wshape, state.wstride)
    return gx, gw


class _Conv1x1Fn(torch.autograd.Function):
    """y = conv2d(x, w) for a bias-free 1x1 stride-1 convolution of a channels_last bf16 or fp16 tensor (fp32 under CONV1X1_F32: the GEMMs of
    conv1x1_f32.hip, mrla_conv1x1_f32_fwd / _wgrad, the same roles), plus the partial
    moment-record rows of y the following BatchNorm needs (mrla_conv1x1_fwd: MRLA_GEMM_MOMENTS records, one row per
    workgroup pixel range -- the resident-weight kernels and the K-streaming kernel of the wide reductions, k >= 512, both
    write them; `mrla_bn_stats_fwd_rows` merges them).  Shapes the GEMMs do not take (mrla_conv1x1_rows < 0) run the stock
    convolution and return no rows; the BatchNorm then takes its own statistics pass.  Backward: dX through the same GEMM on w^T where it applies, dW
    through the split-M GEMM mrla_conv1x1_wgrad; what neither takes stays on the stock convolution backward."""

    @staticmethod
    @_on_device
    def forward(ctx, x, w, want_moments, passthrough=False, w16=None, w16t=None, sub=None, keep=None):
        """w16 / w16t: working copies [n, k] / [k, n], of x's dtype, of an fp32 master weight `w` (WeightBank); the weight gradient
        is then returned in the master's dtype straight from the reduction kernel.
        sub = (sh, sw), with passthrough: the third output is x[:, :, ::sh, ::sw] (dense channels_last) instead of x -- the
        input of the block's strided downsample convolution.  Its gradient then comes back COMPACT, and the input-gradient
        GEMM reads it in place (mrla_conv1x1_fwd_addend) instead of a zero-filled full-size tensor it was scattered into.
        It is an ordinary output of this node: a second consumer, a hook or torch.autograd.grad on it see the true
        gradient of the subsampled tensor, whichever path the backward then takes.
        keep: a list that receives (tensors saved, state) -- for _ConvBnFn, which runs this forward as the first half of
        its own and keeps both on its own context."""
        ctx.set_materialize_grads(False)       # (the moment rows carry no gradient; the shortcut's may be absent)
        outs, saved, ctx.state = _conv1x1_forward(x, w, want_moments, passthrough, w16, w16t, sub)
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(outs[1])
        if keep is not None:
            keep += (saved, ctx.state)
        return outs

    @staticmethod
    @_on_device
    def backward(ctx, dy, _dpart=None, d_through=None):
        return _conv1x1_backward(ctx.saved_tensors, ctx.state, ctx.needs_input_grad[:2], dy, d_through) + (None,) * 6


def _scatter_subsample(g, shape, sh, sw, fmt):
    """The gradient of x[:, :, ::sh, ::sw] in x's shape and memory format: zeros, `g` at the sampled pixels."""
    dx = torch.empty(shape, dtype=g.dtype, device=g.device, memory_format=fmt).zero_()
    dx[:, :, ::sh, ::sw] = g
    return dx


class _SubsampleFn(torch.autograd.Function):
    """x[:, :, ::sh, ::sw] as a dense channels_last tensor, with a backward that stays channels_last: zeros everywhere, the
    incoming gradient at the sampled pixels (autograd's own slice backward answers in NCHW memory, which would cost the
    consumer a full-size layout conversion).  A bottleneck's shortcut does not come through here when conv1 runs on the
    GEMMs: there the subsample is an output of conv1's node (_Conv1x1Fn, sub=...), whose backward needs no full-size tensor."""

    @staticmethod
    def forward(ctx, x, sh, sw):
        ctx.shape, ctx.s = x.shape, (sh, sw)
        # (the memory format of the input is kept: NCHW models stay NCHW)
        ctx.fmt = _CL if x.is_contiguous(memory_format=_CL) and not x.is_contiguous() else torch.contiguous_format
        return x[:, :, ::sh, ::sw].contiguous(memory_format=ctx.fmt)

    @staticmethod
    def backward(ctx, g):
        return _scatter_subsample(g, ctx.shape, ctx.s[0], ctx.s[1], ctx.fmt), None, None


class _ConvBnFn(torch.autograd.Function):
    """relu?(BatchNorm2d(conv1x1(x))) as ONE autograd node, so that its backward can hand the gradient arriving at the
    BatchNorm's output straight to the weight-gradient GEMM (mrla_conv1x1_wgrad_bn): the BatchNorm backward apply pass
    dy = e*dz + f*y + h is formed inside that GEMM, which writes dy once for the input-gradient GEMM -- the tensor between
    the two halves never leaves this node.  The forward IS _Conv1x1Fn's followed by _bn_act_forward, the backward is
    _bn_act_backward and _conv1x1_backward wherever the fused kernel does not apply (frozen weight, a gradient of another
    dtype or layout, an active KernelTimer, WGRAD_BN off): same kernels, same order, same values.  The node keeps the two
    halves' states (_GemmState, _BnActState: no tensors) and one list of saved tensors.
    Outputs: (out[, x']) or, deferred, (y, bnbuf[, x']) -- y the raw convolution output, bnbuf not differentiable; x' the
    passthrough / subsample output of _Conv1x1Fn."""

    @staticmethod
    @_on_device
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, training, momentum, eps, relu, defer, box, passthrough,
                w16, w16t, sub, fuse_dx=False):
        ctx.set_materialize_grads(False)
        ctx.fuse_dx = bool(fuse_dx)
        # (gradients are off inside a forward: this call adds no node, it is _Conv1x1Fn's forward and nothing else.  Through
        # .apply, not the body itself: _Conv1x1Fn.apply is where the GEMM route is observed from outside, for this node too;
        # `kept` brings back what that forward saved and its state)
        kept = []
        res = _Conv1x1Fn.apply(x, w, bool(training), passthrough, w16, w16t, sub, kept)
        gemm_saved, ctx.gemm = kept
        y, part = res[0], res[1]
        out, bn_saved, ctx.bn = _bn_act_forward(y, gamma, beta, running_mean, running_var, training, momentum, eps, relu, defer,
                                                part if part.numel() else None, box)
        ctx.save_for_backward(*gemm_saved, *bn_saved)       # x, w, w16t | y, gamma32, bnbuf
        ctx.nthrough = len(res) - 2
        if defer:
            ctx.mark_non_differentiable(out[1])
            return (y, out[1]) + tuple(res[2:])
        return (out,) + tuple(res[2:]) if len(res) > 2 else out

    @staticmethod
    @_on_device
    def backward(ctx, dy, *rest):
        saved = ctx.saved_tensors
        gemm, bn = ctx.gemm, ctx.bn
        d_through = rest[-1] if ctx.nthrough else None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        x, w, w16t = saved[:3]
        y, gamma32, bnbuf = saved[3:]
        tail = (None,) * 13
        if dy is None:             # only the shortcut carried a gradient
            gx = _conv1x1_backward(saved[:3], gemm, (need_x, need_w), None, d_through)[0]
            return (gx, None, None, None) + tail
        n, k = w.shape
        b, _, h, wd = x.shape
        m = b * h * wd
        lib, dt = L.load(), _DT[x.dtype]
        g = dy if dy.is_contiguous(memory_format=_CL) else None
        fused = (WGRAD_BN and TIMER is None and need_w and g is not None and g.dtype == y.dtype
                 and g.data_ptr() % 16 == 0 and bn.layout == L.NHWC and w.dtype == x.dtype
                 and gemm.wdtype in (x.dtype, torch.float32) and lib.mrla_conv1x1_wgrad_bn_supported(m, k, n, dt) == 1)
        if not fused:              # the two backward passes as they are
            dyc, dgamma, dbeta = _bn_act_backward(saved[3:], bn, dy)
            gx, gw = _conv1x1_backward(saved[:3], gemm, (need_x, need_w), dyc, d_through)
            return (gx, gw, dgamma, dbeta) + tail
        dev, st = x.device, _stream()
        rows = bn.rows
        handed = bn.box.take(g) if bn.box is not None else None           # (sum dz, sum dz*y) taken by the producer of dy
        if handed is not None:
            tmom, rows = handed
        else:
            tmom = torch.empty((rows, n, 2), dtype=torch.float32, device=dev)
        kb = _BnBackward(n, dev)
        mode = L.BN_TRAIN if bn.training else L.BN_EVAL
        if SEQUENCES:              # the sums (unless handed in) and the per-channel constants; no apply pass (dx = NULL)
            L.call("mrla_bn_bwd", _ptr(g), _ptr(y), _ptr(gamma32), _ptr(bnbuf), _ptr(tmom), rows, int(handed is not None),
                   mode, bn.relu, _ptr(kb.small), None, b, n, h, wd, dt, L.NHWC, st)
        else:
            if handed is None:
                L.call("mrla_bn_plane_dmoments", _ptr(g), _ptr(y), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(bnbuf[2]), bn.relu,
                       _ptr(tmom), b, n, h, wd, dt, L.NHWC, st)
            kb.stats(tmom, gamma32, bnbuf, mode, 1, rows, n, m // rows, st)
        prow = lib.mrla_conv1x1_wgrad_rows(m, k, n, dt)
        part = torch.empty((prow, n, k), dtype=torch.float32, device=dev)
        gw = torch.empty((n, k), dtype=gemm.wdtype, device=dev)
        if (WGRAD_BN_DX and ctx.fuse_dx and need_x and d_through is None and gemm.sub is None
                and lib.mrla_conv1x1_wgrad_bn_dx_supported(m, k, n, dt) == 1):
            # dx = dy w inside the same launch: dy never leaves the kernel (wt as _conv1x1_backward takes it)
            wt = w16t if w16t is not None else w.t().contiguous()
            gx = torch.empty_like(x)
            L.call("mrla_conv1x1_wgrad_bn_dx", _ptr(g), _ptr(y), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(kb.small), bn.relu, _ptr(x),
                   _ptr(wt), _ptr(gx), _ptr(part), _ptr(gw), m, k, n, dt, _DT[gemm.wdtype], st)
        else:
            dyc = torch.empty_like(y)
            L.call("mrla_conv1x1_wgrad_bn", _ptr(g), _ptr(y), _ptr(bnbuf[0]), _ptr(bnbuf[1]), _ptr(kb.small), bn.relu, _ptr(dyc),
                   _ptr(x), _ptr(part), _ptr(gw), m, k, n, dt, _DT[gemm.wdtype], st)
            gx = _conv1x1_backward(saved[:3], gemm, (need_x, False), dyc, d_through)[0]
        return (gx, _grad_like(gw, gemm.wshape, gemm.wstride)) + kb.grads(bn.gdtype) + tail


def _conv_bn_fused(conv, bn, x, fused_bn):
    """True when conv + bn on `x` (the GEMM's input) run as the one node _ConvBnFn: a bf16 input, the convolution on the
    forward GEMM, a fused BatchNorm2d behind it, a weight that wants its gradient, and a shape mrla_conv1x1_wgrad_bn takes."""
    if not (WGRAD_BN and TIMER is None and fused_bn and torch.is_grad_enabled() and conv.weight.requires_grad):
        return False
    if x.dtype != torch.bfloat16:      # fp16 keeps the two nodes, as the strided downsample does (conv1x1_applies): the
        return False                   # kernel takes fp16 at the C ABI, the models' fp16 route is pinned pass by pass
    b, k, h, w = x.shape
    lib, m, n, dt = L.load(), b * h * w, conv.out_channels, _DT[x.dtype]
    return lib.mrla_conv1x1_rows(m, k, n, dt) >= 0 and lib.mrla_conv1x1_wgrad_bn_supported(m, k, n, dt) == 1


def _eval_fold_applies(conv, bn, x, fused_bn, defer):
    """True when conv + bn on `x` (the GEMM's input) run as the one launch mrla_conv1x1_fwd_affine: the convolution on the
    forward GEMM, a fused BatchNorm2d in eval mode behind it that is applied here (not deferred), and nothing to
    differentiate -- the rule mrla_light uses for its inference form.  The fold has no backward."""
    if not (EVAL_FOLD and fused_bn and not bn.training and not defer):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, conv.weight, bn.weight, bn.bias)):
        return False
    b, k, h, w = x.shape
    lib, m, n, dt = L.load(), b * h * w, conv.out_channels, _DT[x.dtype]
    return lib.mrla_conv1x1_rows(m, k, n, dt) >= 0 and lib.mrla_conv1x1_fwd_affine_supported(m, k, n, dt) == 1


@functools.partial(_on_device, at=0)                        # (launch where the buffers live)
def _conv_bn_eval_fold(x, w, bn, relu):
    """relu?(bn(conv1x1(x))) for an eval-mode BatchNorm2d in one GEMM launch (no autograd node: _eval_fold_applies).
    x: channels_last [b, k, h, w]; w: the [n, k] (or [n, k, 1, 1]) weight in x's dtype."""
    b, k, h, wd = x.shape
    n, m = w.shape[0], b * h * wd
    dev, st, dt = x.device, _stream(), _DT[x.dtype]
    w = w.detach().reshape(n, k)
    if not w.is_contiguous():
        w = w.contiguous()
    fwd = _BnForward(bn.weight, bn.bias, bn.running_mean, bn.running_var, n, L.BN_EVAL, bn.momentum or 0.0, bn.eps, dev,
                     "conv1x1 + eval-mode BatchNorm")
    bnbuf = fwd.bnbuf
    # (eval mode reads no sums, only the running statistics: one row of one pixel, in a buffer of its own -- the outputs are
    # __restrict__)
    amom = torch.empty((1, n, 2), dtype=torch.float32, device=dev)
    fwd.stats(amom, None, 1, n, 1, st)
    y = torch.empty((b, n, h, wd), dtype=x.dtype, device=dev, memory_format=_CL)
    _call("mrla_conv1x1_fwd_affine", (x.numel() + y.numel()) * x.element_size(), _ptr(x), _ptr(w), _ptr(bnbuf[0]),
          _ptr(bnbuf[1]), int(bool(relu)), _ptr(y), m, k, n, dt, st)
    return y


def _strided_1x1(conv):
    """nn.Conv2d 1x1, no padding, stride > 1 (resnet_mrla_light.py:196-199: the downsample branch of a stage's first block)."""
    return (type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1) and conv.stride != (1, 1)
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None)


def conv1x1_applies(conv, x, strided=False):
    """True when `conv(x)` belongs on the HIP GEMMs: nn.Conv2d 1x1 / stride 1 / no bias, channels_last bf16 or fp16 input,
    and a shape the forward kernel (mrla_conv1x1_rows) or the weight-gradient kernel (mrla_conv1x1_wgrad_rows) takes.
    strided: the question is asked for a strided 1x1 convolution, which runs as the stride-1 GEMM on the subsampled input
    (`x` is the full-size input; the pixel count is the subsampled one).  That question is answered for bf16, and for fp32 under CONV1X1_F32, ONLY: a strided
    fp16 downsample keeps its route -- one stock convolution on the subsampled input (conv_bn_act) -- although the kernels,
    the compact addend of mrla_conv1x1_fwd_addend included, take fp16 at the C ABI; the models do not reach them yet."""
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1) and (strided or conv.stride == (1, 1))
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None):
        return False
    f32 = (CONV1X1_F32 and x.dtype == torch.float32 and conv.weight.dtype == torch.float32
           and not (x.is_cuda and torch.is_autocast_enabled("cuda")))     # (under autocast the convolution is a 16-bit one)
    if not (x.is_cuda and x.dim() == 4 and (f32 or x.dtype in ((torch.bfloat16,) if strided else (torch.bfloat16, torch.float16)))
            and x.is_contiguous(memory_format=_CL)
            and x.data_ptr() % 16 == 0):               # (the kernels move 16-byte fragments)
        return False
    b, k, h, w = x.shape
    if k != conv.in_channels:
        return False
    if strided and strided != "pre":                       # ("pre": `x` is the subsampled input already)
        h, w = (h + conv.stride[0] - 1) // conv.stride[0], (w + conv.stride[1] - 1) // conv.stride[1]
    lib, m, n, dt = L.load(), b * h * w, conv.out_channels, _DT[x.dtype]
    if f32:                     # as below: the forward kernel, or the weight-gradient kernel where a gradient is wanted
        if conv.weight.data_ptr() % 16:
            return False
        if lib.mrla_conv1x1_f32_rows(m, k, n) > 0:
            return True
        return torch.is_grad_enabled() and conv.weight.requires_grad and lib.mrla_conv1x1_f32_wgrad_rows(m, k, n) > 0
    if lib.mrla_conv1x1_rows(m, k, n, dt) >= 0:
        return True
    return torch.is_grad_enabled() and conv.weight.requires_grad and lib.mrla_conv1x1_wgrad_rows(m, k, n, dt) > 0


def _conv_compute_dtype(x):
    """The dtype the stock convolution of `x` computes in: autocast's under CUDA autocast, else x's own."""
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return x.dtype


def _spatial_conv_applies(conv, x, kernel, strides, padding, want_wgrad, dtypes=(torch.bfloat16, torch.float16)):
    """The compute dtype where `conv(x)` is a convolution the own spatial kernels take, else None: a bias-free nn.Conv2d of
    this kernel size and padding, one of `strides`, dilation 1, groups 1, zero padding; a CUDA channels_last 16-byte-aligned
    input of conv's channels that the convolution computes in bf16 or fp16 (its own dtype, or autocast's) on a CUDA weight
    of that dtype (as stored, or as autocast casts it); with `want_wgrad`, grad mode and a weight that wants its gradient.
    `dtypes`: the compute dtypes taken instead of bf16 and fp16."""
    if not (type(conv) is torch.nn.Conv2d and conv.kernel_size == kernel and conv.stride in strides and conv.padding == padding
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"):
        return None
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.is_contiguous(memory_format=_CL) and x.data_ptr() % 16 == 0):
        return None
    wt = conv.weight
    if want_wgrad and not (torch.is_grad_enabled() and wt.requires_grad):
        return None
    if not (wt.is_cuda and x.shape[1] == conv.in_channels):
        return None
    dt, auto = _conv_compute_dtype(x), torch.is_autocast_enabled("cuda")
    if dt not in dtypes or not (x.dtype == dt or (auto and x.dtype == torch.float32)):
        return None
    if not (wt.dtype == dt or (auto and wt.dtype == torch.float32)):       # (the weight as stored, or as autocast casts it)
        return None
    return dt


def _own_wgrad(ctx, entry, rows_entry, dy, x, shape, taps):
    """The weight gradient [n, *taps] of a spatial convolution from its own entry point, in the weight's own dtype and laid
    out as a channels_last [n, c, kh, kw]; None where the kernel does not take the shape (`shape`: the entry point's
    integers in front of the dtype).  The fp32 entry point (an fp32 `x`: _OWN_WGRAD_F32) takes no dtype codes."""
    codes = () if x.dtype == torch.float32 else (_DT[x.dtype], _DT[ctx.wdtype])
    rows = getattr(L.load(), rows_entry)(*shape, *codes[:1])
    if rows <= 0:
        return None
    n, (kh, kw, c) = dy.shape[1], taps
    part = torch.empty((rows, n, kh * kw * c), dtype=torch.float32, device=x.device)
    gw = torch.empty((n, c, kh, kw), dtype=ctx.wdtype, device=x.device, memory_format=_CL)
    _call(entry, (dy.numel() + x.numel()) * x.element_size(), _ptr(dy), _ptr(x), _ptr(part), _ptr(gw), *shape, *codes,
          _stream())
    return gw


def _working_weight(ctx, x, w, for_kernel, banked=None):
    """The weight a spatial convolution node computes on: `w` cast to x's dtype as autocast casts it -- and, where one of the
    own kernels reads it (`for_kernel`: as [n, kh, kw, c], 16 bytes a lane), channels_last and 16-byte aligned; with
    `banked` (Conv3x3Bank.get: (w16, wflip)) that is the bank's copy, the same bits with no kernel launched here.  The
    weight's own shape, strides and dtype are noted on `ctx` for the gradient."""
    ctx.wshape, ctx.wstride, ctx.wdtype = w.shape, w.stride(), w.dtype
    if banked is not None:
        return banked[0]
    w16 = w if w.dtype == x.dtype else w.to(x.dtype)
    if for_kernel:
        w16 = w16.contiguous(memory_format=_CL)
        if w16.data_ptr() % 16:
            w16 = w16.clone(memory_format=_CL)
    return w16


def _weight_strides(ctx, gw):
    """`gw` in the weight's own strides (autograd's / DDP's layout contract)."""
    if gw is not None and gw.stride() != ctx.wstride:
        gw = torch.empty_strided(ctx.wshape, ctx.wstride, dtype=gw.dtype, device=gw.device).copy_(gw)
    return gw


_OWN_WGRAD = {3: ("mrla_conv3x3_wgrad", "mrla_conv3x3_wgrad_rows"), 7: ("mrla_stem_conv_wgrad", "mrla_stem_conv_wgrad_rows")}
_OWN_WGRAD_F32 = {3: ("mrla_conv3x3_f32_wgrad", "mrla_conv3x3_f32_wgrad_rows"),      # an fp32 x and an fp32 weight
                  7: ("mrla_stem_conv_f32_wgrad", "mrla_stem_conv_f32_wgrad_rows")}


def _spatial_conv_backward(ctx, dy, own_wgrad, flipped_dgrad=False, own_dgrad=False):
    """(gx, gw) of a spatial convolution node that saved (x, working weight) and noted ctx.stride: the weight gradient from
    the own kernel if `own_wgrad` (the entry point by x's dtype); the input gradient from the own forward on the flipped,
    transposed weight (a pure permutation) if `flipped_dgrad` at stride 1 -- where the node saved the bank's flipped weight
    behind the two (CONV3X3_DGRAD_FLIP) that one, and without `flipped_dgrad` the stock forward convolution on it --, from
    mrla_conv3x3_dgrad_s2 if `own_dgrad` -- each only for a gradient of x's
    dtype at a 16-byte-aligned address; whatever is asked for and still missing from the stock backward, masked to exactly
    that; the weight gradient in the weight's own dtype and strides (autograd's / DDP's layout contract)."""
    x, w16, *banked_flip = ctx.saved_tensors
    dy = dy.contiguous(memory_format=_CL)
    b, c, h, wd = x.shape
    n, k = w16.shape[0], w16.shape[2]
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    own = dy.dtype == x.dtype and dy.data_ptr() % 16 == 0
    gx = gw = None
    entries = _OWN_WGRAD_F32 if x.dtype == torch.float32 else _OWN_WGRAD
    if need_w and own and own_wgrad and k in entries:
        shape = (b, c, n, h, wd, ctx.stride[0]) if k == 3 else (b, n, h, wd)
        gw = _own_wgrad(ctx, *entries[k], dy, x, shape, (k, k, c))
    if need_x and own and ctx.stride[0] == 1 and (flipped_dgrad or banked_flip):
        # [c, 3, 3, n] in memory: the bank's, or two elementwise kernels
        wflip = banked_flip[0] if banked_flip else w16.flip(2, 3).transpose(0, 1).contiguous(memory_format=_CL)
        if flipped_dgrad:
            gx = torch.empty_like(x)
            _call("mrla_conv3x3_fwd", (dy.numel() + gx.numel()) * x.element_size(), _ptr(dy), _ptr(wflip), _ptr(gx), None,
                  b, n, c, h, wd, 1, _DT[x.dtype], _stream())
        else:              # every element of dX is written: no zero-fill, and the forward solver of the layer's own shape
            gx = torch.ops.aten.convolution(dy, wflip, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1)
    if need_x and own and own_dgrad:
        gx = _own_dgrad_s2(dy, x, w16)
    need_x, need_w = need_x and gx is None, need_w and gw is None
    if need_x or need_w:
        gx2, gw2, _ = torch.ops.aten.convolution_backward(dy, x, w16, None, ctx.stride, (k // 2, k // 2), (1, 1), False, (0, 0),
                                                          1, [need_x, need_w, False])
        gx = gx2 if need_x else gx
        gw = gw2.to(ctx.wdtype) if need_w else gw
    return gx, _weight_strides(ctx, gw)


def conv3x3_applies(conv, x):
    """True when the weight gradient of `conv(x)` belongs on mrla_conv3x3_wgrad: a bias-free nn.Conv2d 3x3 / padding 1 /
    dilation 1 / groups 1 / stride (1, 1) or (2, 2) whose weight wants its gradient, a CUDA channels_last input that the
    convolution computes in bf16 or fp16 (its own dtype, or autocast's), and a shape the kernel takes (mrla_conv3x3_wgrad_rows).
    Frozen stages, ResNeXt groups, dilated detection variants, NCHW and fp32 keep the stock path."""
    dt = _spatial_conv_applies(conv, x, (3, 3), ((1, 1), (2, 2)), (1, 1), True)
    if dt is None:
        return False
    b, c, h, w = x.shape
    return L.load().mrla_conv3x3_wgrad_rows(b, c, conv.out_channels, h, w, conv.stride[0], _DT[dt]) > 0


def conv3x3_f32_applies(conv, x):
    """True when the weight gradient of `conv(x)` belongs on mrla_conv3x3_f32_wgrad: the module conditions of conv3x3_applies
    (a bias-free nn.Conv2d 3x3 / padding 1 / dilation 1 / groups 1 / stride (1, 1) or (2, 2), zero padding), grad mode and an
    fp32 CUDA weight that wants its gradient, a CUDA channels_last 16-byte-aligned fp32 input that the convolution computes
    in fp32 (no autocast), and a shape the kernel takes (mrla_conv3x3_f32_wgrad_rows).  conv3x3_applies goes on answering
    False for all of these."""
    dt = _spatial_conv_applies(conv, x, (3, 3), ((1, 1), (2, 2)), (1, 1), True, dtypes=(torch.float32,))
    if dt is None or x.dtype != torch.float32 or conv.weight.dtype != torch.float32:
        return False
    b, c, h, w = x.shape
    return L.load().mrla_conv3x3_f32_wgrad_rows(b, c, conv.out_channels, h, w, conv.stride[0]) > 0


_WGRAD_PREFERRED = {}      # (b, c, n, h, w, stride, dtype code) -> mrla_conv3x3_wgrad_preferred(...) == 1


def _conv3x3_own_wgrad(conv, x):
    """Whether the weight gradient of `conv(x)` comes from mrla_conv3x3_wgrad: conv3x3_applies, and CONV3X3_WGRAD (everywhere
    the kernel applies) or CONV3X3_WGRAD_AUTO at a shape the library prefers its own kernel at (asked once per shape)."""
    if not ((CONV3X3_WGRAD or CONV3X3_WGRAD_AUTO) and conv3x3_applies(conv, x)):
        return False
    if CONV3X3_WGRAD:
        return True
    b, c, h, w = x.shape
    key = (b, c, conv.out_channels, h, w, conv.stride[0], _DT[_conv_compute_dtype(x)])
    hit = _WGRAD_PREFERRED.get(key)
    if hit is None:
        hit = _WGRAD_PREFERRED[key] = L.load().mrla_conv3x3_wgrad_preferred(*key) == 1
    return hit


def _own_dgrad_s2(dy, x, w16):
    """dX of a stride-2 3x3 convolution from mrla_conv3x3_dgrad_s2 on dy and the forward's own weight `w16` (channels_last
    [n, c, 3, 3] = [n, 3, 3, c] in memory, 16-byte aligned)."""
    b, c, h, wd = x.shape
    gx = torch.empty_like(x)
    _call("mrla_conv3x3_dgrad_s2", (dy.numel() + gx.numel()) * x.element_size(), _ptr(dy), _ptr(w16), _ptr(gx),
          b, c, w16.shape[0], h, wd, _DT[x.dtype], _stream())
    return gx


class _Conv3x3Fn(torch.autograd.Function):
    """y = conv2d(x, w, stride, padding 1) of a channels_last bf16 or fp16 `x` by the stock operator, on `w` cast to x's dtype as
    autocast casts it.  Backward: dW [n, 3, 3, c] from mrla_conv3x3_wgrad where `own_wgrad` (_conv3x3_own_wgrad
    at the call), in the weight's own dtype -- for an fp32 master weight the fp32 sums themselves, no 16-bit rounding and no
    cast kernel -- returned as [n, c, 3, 3]; dX from mrla_conv3x3_dgrad_s2 where `own_dgrad` (CONV3X3_DGRAD and
    conv3x3_dgrad_applies at the call); what is left from the stock operator's backward, masked to exactly that (its split-K
    weight-gradient solver is never invoked under `own_wgrad`).  An fp32 `x` with an fp32 `w` (CONV3X3_WGRAD_F32 and
    conv3x3_f32_applies at the call) is the same node: dW then comes from mrla_conv3x3_f32_wgrad."""

    @staticmethod
    @_on_device
    def forward(ctx, x, w, stride, own_wgrad, own_dgrad, banked):
        ctx.stride, ctx.own_wgrad, ctx.own_dgrad = (stride, stride), own_wgrad, own_dgrad
        w16 = _working_weight(ctx, x, w, own_dgrad, banked)
        ctx.save_for_backward(x, w16, *(() if banked is None else banked[1:]))
        return torch.ops.aten.convolution(x, w16, None, ctx.stride, (1, 1), (1, 1), False, (0, 0), 1)

    @staticmethod
    @_on_device
    def backward(ctx, dy):
        return _spatial_conv_backward(ctx, dy, own_wgrad=ctx.own_wgrad, own_dgrad=ctx.own_dgrad) + (None,) * 4


def conv3x3_fwd_applies(conv, x):
    """True when `conv(x)` itself belongs on mrla_conv3x3_fwd: the module, layout, dtype and shape conditions of
    conv3x3_applies (a bias-free nn.Conv2d 3x3 / padding 1 / dilation 1 / groups 1 / stride (1, 1) or (2, 2), a CUDA
    channels_last 16-byte-aligned input computed in bf16 or fp16, a shape the kernel takes: mrla_conv3x3_fwd_rows) -- but
    neither grad mode nor a weight that wants its gradient: inference and frozen stages qualify."""
    dt = _spatial_conv_applies(conv, x, (3, 3), ((1, 1), (2, 2)), (1, 1), False)
    if dt is None:
        return False
    b, c, h, w = x.shape
    return L.load().mrla_conv3x3_fwd_rows(b, c, conv.out_channels, h, w, conv.stride[0], _DT[dt]) > 0


def conv3x3_dgrad_applies(conv, x):
    """True when the input gradient of `conv(x)` belongs on mrla_conv3x3_dgrad_s2: the module, layout and dtype conditions of
    conv3x3_fwd_applies, stride (2, 2), grad mode and an input that wants its gradient, and a shape the kernel takes
    (mrla_conv3x3_dgrad_s2_plan).  A frozen weight qualifies; stride 1 has its own route (CONV3X3_FWD)."""
    dt = _spatial_conv_applies(conv, x, (3, 3), ((2, 2),), (1, 1), False)
    if dt is None or not (torch.is_grad_enabled() and x.requires_grad):
        return False
    b, c, h, w = x.shape
    return L.conv3x3_dgrad_s2_plan(b, c, conv.out_channels, h, w, _DT[dt]) is not None


class _Conv3x3FwdFn(torch.autograd.Function):
    """(y, records) = mrla_conv3x3_fwd of a channels_last bf16 or fp16 `x` on `w` cast to x's dtype as autocast casts it and
    laid out [n, 3, 3, c]; records: the [rows, n, MRLA_GEMM_MOMENTS] moment records of y for the BatchNorm behind it where
    `moments`, else empty.  Backward: dX at stride 1 from the same entry point on dy and the flipped, transposed weight (a
    pure permutation), at stride 2 from mrla_conv3x3_dgrad_s2 on dy and the saved weight itself where `own_dgrad`
    (CONV3X3_DGRAD and conv3x3_dgrad_applies at the call), else from the stock operator's backward; dW from
    mrla_conv3x3_wgrad where `own_wgrad` (_conv3x3_own_wgrad at the call), else from the stock backward --
    each masked to what is asked for."""

    @staticmethod
    @_on_device
    def forward(ctx, x, w, stride, moments, own_wgrad, own_dgrad, banked):
        ctx.set_materialize_grads(False)
        ctx.stride, ctx.own_wgrad, ctx.own_dgrad = (stride, stride), own_wgrad, own_dgrad
        w16 = _working_weight(ctx, x, w, True, banked)
        b, c, h, wd = x.shape
        n, dt = w16.shape[0], _DT[x.dtype]
        ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
        y = torch.empty((b, n, ho, wo), dtype=x.dtype, device=x.device, memory_format=_CL)
        if moments:
            rows = L.load().mrla_conv3x3_fwd_rows(b, c, n, h, wd, stride, dt)
            part = torch.empty((max(rows, 0), n, L.GEMM_MOMENTS), dtype=torch.float32, device=x.device)
        else:
            part = torch.empty((0,), dtype=torch.float32, device=x.device)
        _call("mrla_conv3x3_fwd", (x.numel() + y.numel()) * x.element_size(), _ptr(x), _ptr(w16), _ptr(y),
              _ptr(part) if moments else None, b, c, n, h, wd, stride, dt, _stream())
        ctx.save_for_backward(x, w16, *(() if banked is None else banked[1:]))
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    @_on_device
    def backward(ctx, dy, _dpart=None):
        if dy is None:
            return (None,) * 7
        return _spatial_conv_backward(ctx, dy, own_wgrad=ctx.own_wgrad, flipped_dgrad=True, own_dgrad=ctx.own_dgrad) + (None,) * 5


_DGRAD_FLIP_PREFERRED = {}      # (b, c, n, h, w, dtype code) -> mrla_conv3x3_dgrad_flip_preferred(...) == 1


def _conv3x3_banked(conv, x, by_rule):
    """(w16, wflip) of `conv` from the Conv3x3Bank of the running forward, refreshed for it -- or None: CONV3X3_DGRAD_FLIP
    off, no bank (a call outside a model's bookkeeping), not a stride-1 convolution the own spatial kernels' module, layout
    and dtype conditions hold for, grad mode off or an input that wants no gradient, a weight the bank does not take, and,
    `by_rule`, a shape mrla_conv3x3_dgrad_flip_preferred answers 0 for (asked once per shape)."""
    book = current_bookkeeping()
    if not CONV3X3_DGRAD_FLIP or book is None or book.bank3 is None:
        return None
    dt = _spatial_conv_applies(conv, x, (3, 3), ((1, 1),), (1, 1), False)
    if dt is None or not (torch.is_grad_enabled() and x.requires_grad):
        return None
    if by_rule:
        b, c, h, w = x.shape
        key = (b, c, conv.out_channels, h, w, _DT[dt])
        hit = _DGRAD_FLIP_PREFERRED.get(key)
        if hit is None:
            hit = _DGRAD_FLIP_PREFERRED[key] = L.load().mrla_conv3x3_dgrad_flip_preferred(*key) == 1
        if not hit:
            return None
    return book.bank3.get(conv, dt, book)


def _conv3x3_own(x, conv, moments):
    dt = _conv_compute_dtype(x)
    return _Conv3x3FwdFn.apply(x if x.dtype == dt else x.to(dt), conv.weight, conv.stride[0], moments,
                               _conv3x3_own_wgrad(conv, x), CONV3X3_DGRAD and conv3x3_dgrad_applies(conv, x),
                               _conv3x3_banked(conv, x, False))


def conv3x3(x, conv):
    """conv(x) for the 3x3 convolutions of the blocks (resnet_mrla_light.py: conv2 of the bottleneck, both of the basic
    block).  With CONV3X3_FWD on and conv3x3_fwd_applies: one autograd node on mrla_conv3x3_fwd (_Conv3x3FwdFn).  Else, where
    neither the own weight gradient (conv3x3_applies, and CONV3X3_WGRAD or CONV3X3_WGRAD_AUTO at a shape
    mrla_conv3x3_wgrad_preferred answers 1 for; in fp32 conv3x3_f32_applies and CONV3X3_WGRAD_F32) nor CONV3X3_DGRAD with
    conv3x3_dgrad_applies holds, nor the stride-1 input gradient is routed to the stock forward on the banked flipped weight
    (CONV3X3_DGRAD_FLIP: _conv3x3_banked), it IS conv(x): the same autograd graph as before.  Otherwise one autograd node (_Conv3x3Fn)
    whose forward is the stock operator's, whose weight gradient is mrla_conv3x3_wgrad's (fp32: mrla_conv3x3_f32_wgrad's)
    under the first and whose input gradient is mrla_conv3x3_dgrad_s2's under the second."""
    if CONV3X3_FWD and conv3x3_fwd_applies(conv, x):
        return _conv3x3_own(x, conv, False)[0]
    own_wgrad = _conv3x3_own_wgrad(conv, x) or (CONV3X3_WGRAD_F32 and conv3x3_f32_applies(conv, x))
    own_dgrad = CONV3X3_DGRAD and conv3x3_dgrad_applies(conv, x)
    banked = _conv3x3_banked(conv, x, True)
    if not (own_wgrad or own_dgrad or banked):
        return conv(x)
    dt = _conv_compute_dtype(x)
    return _Conv3x3Fn.apply(x if x.dtype == dt else x.to(dt), conv.weight, conv.stride[0], own_wgrad, own_dgrad, banked)


def conv3x3_bn_act(x, conv, bn, relu, defer=False):
    """bn_act(conv3x3(x, conv), bn, relu, defer) -- and exactly that graph with CONV3X3_FWD off or where conv3x3_fwd_applies says
    no.  With the own forward in front of a train-mode BatchNorm2d that bn_act fuses, the convolution also returns the moment
    records of its output and bn_act takes them as `pre_moments` (the path the 1x1 GEMMs feed): no moments pass reads y back."""
    if CONV3X3_FWD and conv3x3_fwd_applies(conv, x):
        moments = _is_fused_bn(bn) and bn.training
        y, part = _conv3x3_own(x, conv, moments)
        return bn_act(y, bn, relu, defer, pre_moments=part if moments else None)
    return bn_act(conv3x3(x, conv), bn, relu, defer)


def stem_conv_applies(conv, x):
    """True when the weight gradient of `conv(x)` belongs on mrla_stem_conv_wgrad: a bias-free nn.Conv2d 7x7 / stride (2, 2) /
    padding (3, 3) / dilation 1 / groups 1 of three input channels whose weight wants its gradient, a CUDA channels_last
    16-byte-aligned input that the convolution computes in bf16 or fp16 (its own dtype, or autocast's), and a shape the kernel
    takes (mrla_stem_conv_wgrad_rows).  Everything else keeps the stock path."""
    dt = _spatial_conv_applies(conv, x, (7, 7), ((2, 2),), (3, 3), True)
    if dt is None or conv.in_channels != 3:
        return False
    b, _, h, w = x.shape
    return L.load().mrla_stem_conv_wgrad_rows(b, conv.out_channels, h, w, _DT[dt]) > 0


def stem_conv_f32_applies(conv, x):
    """True when the weight gradient of `conv(x)` belongs on mrla_stem_conv_f32_wgrad: the module conditions of
    stem_conv_applies (a bias-free nn.Conv2d 7x7 / stride (2, 2) / padding (3, 3) / dilation 1 / groups 1 of three input
    channels, zero padding), grad mode and an fp32 CUDA weight that wants its gradient, a CUDA channels_last 16-byte-aligned
    fp32 input that the convolution computes in fp32 (no autocast), and a shape the kernel takes
    (mrla_stem_conv_f32_wgrad_rows).  stem_conv_applies goes on answering False for all of these."""
    dt = _spatial_conv_applies(conv, x, (7, 7), ((2, 2),), (3, 3), True, dtypes=(torch.float32,))
    if dt is None or conv.in_channels != 3 or x.dtype != torch.float32 or conv.weight.dtype != torch.float32:
        return False
    b, _, h, w = x.shape
    return L.load().mrla_stem_conv_f32_wgrad_rows(b, conv.out_channels, h, w) > 0


class _StemConvFn(torch.autograd.Function):
    """y = conv2d(x, w, stride 2, padding 3) of a channels_last bf16 or fp16 three-channel `x` by the stock operator, on `w`
    cast to x's dtype as autocast casts it.  Backward: dW [n, 7, 7, 3] from mrla_stem_conv_wgrad in the weight's own dtype --
    for an fp32 master weight the fp32 sums themselves -- returned as [n, 3, 7, 7] with the weight's strides.  The stock
    backward runs only for what is left: dX if `x` itself needs a gradient (the image batch does not), and dW where dy arrives
    in another dtype or misaligned.  An fp32 `x` with an fp32 `w` (STEM_WGRAD_F32 and stem_conv_f32_applies at the call) is
    the same node: dW then comes from mrla_stem_conv_f32_wgrad."""

    @staticmethod
    @_on_device
    def forward(ctx, x, w):
        ctx.stride = (2, 2)
        w16 = _working_weight(ctx, x, w, False)
        ctx.save_for_backward(x, w16)
        return torch.ops.aten.convolution(x, w16, None, ctx.stride, (3, 3), (1, 1), False, (0, 0), 1)

    @staticmethod
    @_on_device
    def backward(ctx, dy):
        return _spatial_conv_backward(ctx, dy, own_wgrad=True)


def stem_conv(x, conv):
    """conv(x) for the stem's 7x7 / stride 2 convolution (resnet_mrla_light.py: conv1).  Where neither STEM_WGRAD with
    stem_conv_applies nor STEM_WGRAD_F32 with stem_conv_f32_applies holds, it IS conv(x): the same autograd graph as before.
    Otherwise one autograd node whose forward is the stock operator's and whose weight gradient is mrla_stem_conv_wgrad's
    (fp32: mrla_stem_conv_f32_wgrad's)."""
    if not ((STEM_WGRAD and stem_conv_applies(conv, x)) or (STEM_WGRAD_F32 and stem_conv_f32_applies(conv, x))):
        return conv(x)
    dt = _conv_compute_dtype(x)
    return _StemConvFn.apply(x if x.dtype == dt else x.to(dt), conv.weight)


def shortcut_subsample(downsample, x):
    """(sh, sw) when `downsample` is the strided 1x1 convolution + BatchNorm of a stage's first block
    (resnet_mrla_light.py:196-199) and runs on the GEMMs for the block input `x` (bf16, or fp32 under CONV1X1_F32: conv1x1_applies), else None.
    The block then asks conv1 for
    the subsampled input (conv_bn_act(..., passthrough=True, subsample=...)) and hands it on with presampled=True."""
    if not (isinstance(downsample, torch.nn.Sequential) and len(downsample) == 2 and _strided_1x1(downsample[0])):
        return None
    if not (torch.is_tensor(x) and x.dim() == 4 and conv1x1_applies(downsample[0], x, True)):
        return None
    return tuple(downsample[0].stride)


def _gemm_weights(conv, x):
    """(weight, w16, w16t) for _Conv1x1Fn / _ConvBnFn on the input `x`: the module's weight, and -- when it is an fp32 master
    of a 16-bit `x` -- the step's working copy in x's dtype and its transpose from the WeightBank, or the weight cast as
    autocast would cast it for the stock convolution (differentiable)."""
    wt, w16, w16t = conv.weight, None, None
    if wt.dtype != x.dtype:
        book = current_bookkeeping()
        held = book.bank.get(conv, x.dtype) if (book is not None and book.bank is not None and wt.dtype == torch.float32) else None
        if held is not None:
            w16, w16t = held
        else:
            wt = wt.to(x.dtype)
    return wt, w16, w16t


def conv_bn_act(x, conv, bn, relu, defer=False, passthrough=False, subsample=None, presampled=False, fuse_dx=False):
    """relu?(bn(conv(x))) -- resnet_mrla_light.py:93-94,100-101.  Eligible 1x1 convolutions run on the HIP GEMM, whose
    epilogue hands the train-mode BatchNorm its statistics (the moments pass over the output disappears); everything
    else is `bn_act(conv(x), ...)` with the stock convolution.
    passthrough=True returns (result, x'), x' being x routed through the convolution's autograd node: a consumer that
    uses x' as the block's shortcut (resnet_mrla_light.py:91,110-114) gets the shortcut gradient added inside the
    convolution's input-gradient GEMM instead of by a separate accumulation pass.
    subsample=(sh, sw), with passthrough: x' is x[:, :, ::sh, ::sw] routed the same way -- the input of the block's strided
    downsample convolution (shortcut_subsample), whose input gradient then reaches the GEMM compact instead of scattered
    into a zero-filled tensor of x's size.  presampled=True: `conv` is that strided 1x1 convolution and `x` the already
    subsampled input.
    fuse_dx=True: where the pair runs as the one node _ConvBnFn and the shape allows it, the backward forms the input gradient
    inside the weight-gradient launch as well (WGRAD_BN_DX, mrla_conv1x1_wgrad_bn_dx) -- the same values bit for bit; the
    bottleneck asks for it on conv3 and the downsample.  Without it the backward launches what it always launched."""
    def second(t):                  # the second result where the convolution's own node does not produce it
        return _SubsampleFn.apply(t, subsample[0], subsample[1]) if subsample is not None else t

    fused_bn = _is_fused_bn(bn)
    # A strided 1x1 convolution is the stride-1 one on the subsampled input: one strided copy (a quarter of the pixels), then
    # the same GEMMs -- forward with the BatchNorm statistics in its epilogue, input gradient, weight gradient.  Not for speed
    # alone: MIOpen's input gradient of exactly these convolutions is right when launched eagerly and garbage from the second
    # replay of a HIP graph on (every mode: immediate, find, deterministic; scripts/miopen_bwd_graph_probe.py,
    # profiles/r05_notes.md section 2) -- with them on the GEMMs the whole step replays correctly.
    strided = (_strided_1x1(conv) and not passthrough and x.dim() == 4
               and conv1x1_applies(conv, x, "pre" if presampled else True))
    if strided or conv1x1_applies(conv, x):
        if strided and not presampled:
            x = _SubsampleFn.apply(x, conv.stride[0], conv.stride[1])
        wt, w16, w16t = _gemm_weights(conv, x)
        if _eval_fold_applies(conv, bn, x, fused_bn, defer):
            # (`x` is the subsampled input of a strided downsample here; passthrough: as the route without a GEMM node below)
            out = _conv_bn_eval_fold(x.detach(), w16 if w16 is not None else wt, bn, relu)
            return (out, second(x)) if passthrough else out
        if _conv_bn_fused(conv, bn, x, fused_bn):
            training, momentum = _bn_step(bn)
            box = _DeferredBnBox() if defer else None
            through = passthrough and x.requires_grad
            res = _ConvBnFn.apply(x, wt, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum,
                                  bn.eps, relu, defer, box, through, w16, w16t, subsample if through else None, fuse_dx)
            res = res if isinstance(res, tuple) else (res,)
            out = res[0]
            if defer:
                out._mrla_affine = (res[1][0], res[1][1])
                out._mrla_bn_box = box
            if not passthrough:
                return out
            return out, (res[-1] if through else second(x))
        if passthrough and torch.is_grad_enabled() and x.requires_grad:
            y, part, through = _Conv1x1Fn.apply(x, wt, bool(fused_bn and bn.training), True, w16, w16t, subsample)
            return bn_act(y, bn, relu, defer, pre_moments=part if part.numel() else None), through
        y, part = _Conv1x1Fn.apply(x, wt, bool(fused_bn and bn.training), False, w16, w16t)
        out = bn_act(y, bn, relu, defer, pre_moments=part if part.numel() else None)
        return (out, second(x)) if passthrough else out
    if presampled:                  # (not reached from the models: shortcut_subsample() asked conv1x1_applies first)
        return bn_act(torch.nn.functional.conv2d(x, conv.weight), bn, relu, defer)
    if _strided_1x1(conv) and not passthrough and x.dim() == 4 and x.is_cuda:
        # every other dtype / layout (resnet/train.py itself trains in fp32, :397-409): still the stride-1 convolution on the
        # subsampled input -- a plain GEMM for MIOpen, whose input gradient needs no zero-fill + scatter; the zero-fill and
        # the strided copy of _SubsampleFn are ordinary captured kernels.  (F.conv2d: autocast casts as for the module.)
        xs = _SubsampleFn.apply(x, conv.stride[0], conv.stride[1])
        return bn_act(torch.nn.functional.conv2d(xs, conv.weight), bn, relu, defer)
    out = bn_act(conv(x), bn, relu, defer)
    return (out, second(x)) if passthrough else out


def conv_bn_gate(x, conv, bn, se=None, eca=None):
    """eca?(se?(bn(conv(x)))) -- resnet_mrla_light.py:101-108 (conv3, bn3, then the block's channel attention).  Where the
    BatchNorm + gate node applies to the convolution's output (bn_gate_applies) the convolution runs bare -- an eligible 1x1
    on the HIP GEMM without moment records: the node's plane-moments pass, which it needs for the pool anyway, supplies the
    statistics -- and bn_gate does the rest; otherwise conv_bn_act as without a gate, then the eager modules."""
    if x.dim() == 4 and type(conv) is torch.nn.Conv2d:
        cl = x.is_contiguous(memory_format=_CL)
        ho = (x.shape[2] + 2 * conv.padding[0] - conv.dilation[0] * (conv.kernel_size[0] - 1) - 1) // conv.stride[0] + 1
        wo = (x.shape[3] + 2 * conv.padding[1] - conv.dilation[1] * (conv.kernel_size[1] - 1) - 1) // conv.stride[1] + 1
        odt = torch.get_autocast_dtype("cuda") if (x.is_cuda and torch.is_autocast_enabled("cuda")) else x.dtype
        if bn_gate_applies((x.shape[0], conv.out_channels, ho, wo), odt, cl, x.is_cuda, bn, se, eca):
            if conv1x1_applies(conv, x):
                wt, w16, w16t = _gemm_weights(conv, x)
                y, _ = _Conv1x1Fn.apply(x, wt, False, False, w16, w16t)
            else:
                y = conv(x)
            return bn_gate(y, bn, se, eca)
    out = conv_bn_act(x, conv, bn, relu=False)
    if se is not None:
        out = se(out)
    if eca is not None:
        out = eca(out)
    return out
