"""Autograd functions over the HIP kernels of libimgcomp.so.

Every forward/backward here launches hand-written gfx950 kernels through the
C ABI (include/imgcomp.h) on torch's current stream.  PyTorch provides only
allocation (caching allocator), stream handles and the autograd graph.
There is deliberately no CPU / eager fallback: CPU tensors raise.

Layout convention: activations with >= 32 channels live in NHWC
(torch.channels_last) so every GEMM operand row is channel-contiguous; the
3-channel image tensors stay NCHW and take the generic gather path.
"""
import os
import threading
import weakref

import torch
from torch.autograd import Function

from . import _lib
from . import noise as _noise

CL = torch.channels_last


def _cl(t):
    """Channels-last (NHWC) dense view/copy for GEMM operands with many channels."""
    if t.shape[1] >= 32 and t.stride(1) != 1:
        return t.contiguous(memory_format=CL)
    if not (t.is_contiguous() or t.is_contiguous(memory_format=CL)):
        return t.contiguous()
    return t


def _new_act(N, C, H, W, device):
    if C >= 32:
        return torch.empty((N, C, H, W), device=device, dtype=torch.float32, memory_format=CL)
    return torch.empty((N, C, H, W), device=device, dtype=torch.float32)


def _is_dense(t):
    """Non-overlapping and dense storage in some dimension order."""
    if t.numel() <= 1:
        return True
    expect = 1
    for s, n in sorted((s, n) for s, n in zip(t.stride(), t.shape) if n != 1):
        if s != expect:
            return False
        expect *= n
    return True


def _dense(t):
    if t.is_contiguous() or _is_dense(t):
        return t
    return t.contiguous()


def _match(g, ref):
    """Return g with exactly ref's strides (elementwise kernels index storage)."""
    if g.shape == ref.shape and g.stride() == ref.stride() and _is_dense(g):
        return g
    out = torch.empty_like(ref)
    out.copy_(g)
    return out


# launch-plan log (tests): while a list is installed by `record_plans`, every conv / GDN op
# appends the plan (ic_conv_plan) of each launch it makes, so a test can show which kernel
# instances a whole training step ran
_PLAN_LOG = None


class record_plans:
    def __enter__(self):
        global _PLAN_LOG
        self.log, _PLAN_LOG = [], []
        return _PLAN_LOG

    def __exit__(self, *exc):
        global _PLAN_LOG
        _PLAN_LOG = None
        return False


def _log_plan(op, a, b, k=1, stride=1, pad=0, math=0):
    if _PLAN_LOG is not None:
        _PLAN_LOG.append(dict(_lib.plan(op, a, b, k, stride, pad, math), op=op))


# ============================================================== convolutions
# Column sums of a gradient computed by the op that produced it (GDN backward: sum over pixels
# of dx), handed to the conv whose output received that gradient, which then skips its own
# bias-gradient pass over the same tensor.  Keyed by the gradient tensor itself (device +
# storage pointer, checked against a weakref and the version counter): a gradient changed in
# between (or any other tensor) falls back to the pass.  Backward passes of several devices may
# run concurrently (one autograd thread per device; nn.DataParallel replicas), so the table is
# locked.
class _Handoff:
    """Payloads handed from the op that produced a tensor to the op that receives it (see above, and the
    bf16 copies below): put(t, payload), then take(t) once, by the same tensor at the same version."""

    def __init__(self):
        self._entries = {}
        self._lock = threading.Lock()
        self.stats = {"put": 0, "hit": 0}

    @staticmethod
    def _key(t):
        return (t.device.index, t.data_ptr())

    def put(self, t, payload):
        with self._lock:
            for k in [k for k, (r, _, _) in self._entries.items() if r() is None]:
                del self._entries[k]
            self._entries[self._key(t)] = (weakref.ref(t), t._version, payload)
            self.stats["put"] += 1

    def take(self, t, fits=None):
        """The payload put for t, or None; fits(payload): a further condition of a hit."""
        with self._lock:
            e = self._entries.pop(self._key(t), None)
        if e is None:
            return None
        r, ver, payload = e
        if r() is t and t._version == ver and (fits is None or fits(payload)):
            self.stats["hit"] += 1
            return payload
        return None


_COLSUMS = _Handoff()
_put_colsum, _take_colsum = _COLSUMS.put, _COLSUMS.take


# ---------------------------------------------------------- bf16 activation copies (config C3)
# A GDN whose output feeds a conv forward on the bf16 DMA tiles (GDN.xb & 1), or whose input
# gradient feeds a transposed conv's input gradient there (GDN.xb & 2), writes that tensor's compact
# NHWC bf16 copy in the same kernel (torch.ops.imgcomp.gdn_fwd_xb / gdn_bwd_sum_xb) and leaves it
# here, keyed like the column sums above; the consuming conv takes it (conv2d_fwd_xb /
# conv_transpose2d_dgrad_xb) and reads 2 B per element instead of converting the fp32 tensor.
_BF16 = _Handoff()
BF16_COPY_STATS = _BF16.stats
_put_bf16 = _BF16.put


def _take_bf16(t):
    return _BF16.take(t, lambda tb: tb.shape == t.shape and tb.stride() == t.stride())


# torch.nn.Conv2d (analysis.py:55, prior_analysis.py:54-56) and torch.nn.ConvTranspose2d (synthesis.py:55-57,
# prior_synthesis.py:54-56): one forward and one backward for both, each launch one torch.ops.imgcomp op
# (csrc/torch_ops.cpp -> C ABI).  A transposed conv differs in its ops' names, in the weight dimension that
# matches the input's channels (0, not 1), and in taking an output_padding after stride and padding.
_CONV_OP = {False: "conv2d", True: "conv_transpose2d"}


def _conv_forward(ctx, transposed, x, weight, bias, geom, act, math):
    _lib.require_device(x, weight, bias)
    x = _cl(x)
    w = weight.contiguous()
    b = None if bias is None else bias.contiguous()
    op = _CONV_OP[transposed]
    if w.shape[0 if transposed else 1] != x.shape[1] or w.shape[2] != w.shape[3]:
        raise RuntimeError(f"{op}: weight {tuple(w.shape)} does not match input {tuple(x.shape)}")
    xb = _take_bf16(x) if int(math) & MATH["bf16"] else None
    if xb is not None:
        y = getattr(_lib.ops(), op + "_fwd_xb")(x, xb, w, b, *geom, int(act), int(math))
    else:
        y = getattr(_lib.ops(), op + "_fwd")(x, w, b, *geom, int(act), int(math))
    stride, padding = geom[:2]
    _log_plan(op + "_fwd", x, y, w.shape[2], stride, padding, math)
    # x's bf16 copy, for the weight gradient with dy's (*_wgrad_xb); held to the backward
    # (2 B per element of x) only when that weight gradient will run
    ctx.xb = xb if ctx.needs_input_grad[1] else None
    ctx.conf = (stride, padding, act, b is not None, int(math))
    ctx.save_for_backward(x, w, y if act else None)
    return y


def _conv_backward(ctx, transposed, gy):
    """(dx, dw, db)"""
    x, w, y = ctx.saved_tensors
    stride, padding, act, has_b, math = ctx.conf
    # the bias gradient formed by gy's producer (taken only where this node owns the bias gradient)
    pre = _take_colsum(gy) if (has_b and not act and ctx.needs_input_grad[2]) else None
    gyb = _take_bf16(gy) if (math & MATH["bf16"]) and not act else None
    if act:
        gy = relu_bwd(y, gy)
    gy = _cl(gy)
    dx = dw = db = None
    ops, op, k = _lib.ops(), _CONV_OP[transposed], w.shape[2]
    if ctx.needs_input_grad[0]:
        if gyb is not None and gyb.stride() == gy.stride():
            dx = getattr(ops, op + "_dgrad_xb")(gy, gyb, w, x, stride, padding, math)
        else:
            dx = getattr(ops, op + "_dgrad")(gy, w, x, stride, padding, math)
        _log_plan(op + "_dgrad", gy, dx, k, stride, padding, math)
    if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
        xb, ctx.xb = ctx.xb, None
        if xb is not None and gyb is not None and gyb.stride() == gy.stride():
            dw, db = getattr(ops, op + "_wgrad_xb")(x, xb, gy, gyb, w, stride, padding, has_b and pre is None, math)
        else:
            dw, db = getattr(ops, op + "_wgrad")(x, gy, w, stride, padding, has_b and pre is None, math)
        _log_plan(op + "_wgrad", x, gy, k, stride, padding, math)
        db = (db if pre is None else pre) if has_b else None
    return dx, dw, db


class Conv2dFn(Function):
    transposed = False

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, act, math=0):
        return _conv_forward(ctx, False, x, weight, bias, (stride, padding), act, math)

    @staticmethod
    def backward(ctx, gy):
        return _conv_backward(ctx, False, gy) + (None,) * 4


class ConvTranspose2dFn(Function):
    transposed = True

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, output_padding, act, math=0):
        return _conv_forward(ctx, True, x, weight, bias, (stride, padding, output_padding), act, math)

    @staticmethod
    def backward(ctx, gy):
        return _conv_backward(ctx, True, gy) + (None,) * 5


# include/imgcomp.h IC_MATH_*: "fp32" exact fp32 MFMA; "bf16" bf16 operands, fp32 accumulation
# (reduced precision, config C3); "fp32_split" fp32 arithmetic on the bf16 MFMA through an exact
# three-term bf16 split of both operands (six products, error of an fp32 fma chain)
MATH = {"fp32": 0, "bf16": 1, "fp32_split": 2}


# ---------------------------------------------------------- eval-mode weight caching
# Inside `weight_cache()` (Evaluator.run_eval's eager path; GraphForward does not enter it: a
# captured graph already holds its pack launches), forwards without autograd keep each
# conv weight's MFMA pack in a workspace of its own and skip the pack launch while the weight is
# unchanged (include/imgcomp.h IC_MATH_WPACKED), and NonNegativeParam keeps its re-parameterised
# value: the eval forward then launches only the layer kernels.  An entry is valid for the same
# tensor object (weakref) at the same version counter (every in-place update bumps it: torch ops,
# load_state_dict's copy_, and solver.AdamW, which bumps it after its kernel) on the same stream
# (the pack workspace also holds the split-K partials) and, for packs, the same operand geometry.
# The stream is keyed by its raw handle: a stream destroyed inside one scope whose handle is reused
# by a new stream would find the old entry, but the weakref and version checks still decide a hit,
# and every entry is dropped when the outermost scope exits.
IC_MATH_WPACKED = 4
_WCACHE = {}
_WCACHE_LOCK = threading.Lock()
_WCACHE_DEPTH = [0]


class weight_cache:
    """Scope in which no-grad forwards reuse weight packs and re-parameterisations.  Entries are
    dropped when the outermost scope exits."""

    def __enter__(self):
        with _WCACHE_LOCK:
            _WCACHE_DEPTH[0] += 1
        return self

    def __exit__(self, *exc):
        with _WCACHE_LOCK:
            _WCACHE_DEPTH[0] -= 1
            if _WCACHE_DEPTH[0] == 0:
                _WCACHE.clear()
        return False


def _wcache_on(t):
    return _WCACHE_DEPTH[0] > 0 and not torch.is_grad_enabled() and t.is_cuda


def _wcache_get(kind, t, geom):
    """(entry dict, hit) for tensor t; the entry is reset unless t, its version and geom match."""
    stream = torch.cuda.current_stream(t.device).cuda_stream
    key = (kind, t.device.index, t.data_ptr(), stream, geom)  # one entry per geometry (portrait / landscape)
    with _WCACHE_LOCK:
        for k in [k for k, e in _WCACHE.items() if e["ref"]() is None]:
            del _WCACHE[k]
        e = _WCACHE.get(key)
        hit = e is not None and e["ref"]() is t and e["ver"] == t._version
        if not hit:
            ws = e.get("ws") if e is not None else None  # keep the (grown) workspace
            e = {"ref": weakref.ref(t), "ver": t._version}
            if ws is not None:
                e["ws"] = ws
            _WCACHE[key] = e
        return e, hit


def _cached_conv(op, x, weight, bias, args, math):
    _lib.require_device(x, weight, bias)
    x = _cl(x)
    w = weight.contiguous()
    b = None if bias is None else bias.contiguous()
    geom = (op, tuple(x.shape), tuple(x.stride()), tuple(w.shape), args, int(math))
    e, hit = _wcache_get("pack", weight, geom)
    if "ws" not in e:
        e["ws"] = torch.empty(16, dtype=torch.uint8, device=x.device)
    m = int(math) | (IC_MATH_WPACKED if hit else 0)
    fn = getattr(_lib.ops(), op)
    y = fn(x, w, b, *args, m, e["ws"])
    _log_plan(op.replace("_ws", ""), x, y, w.shape[2], args[0], args[1], math)
    return y


def nonneg_cached(p, bound, pedestal):
    """NonNegFn.apply(p, ...) kept per (tensor, version) inside `weight_cache()`."""
    if not _wcache_on(p):
        return NonNegFn.apply(p, bound, pedestal)
    e, hit = _wcache_get("nonneg", p, (float(bound), float(pedestal)))
    if not hit or "val" not in e:
        e["val"] = NonNegFn.apply(p, bound, pedestal)
    return e["val"]


# ---------------------------------------------------------- weight gradients on a stream of their own
# A conv whose forward runs on a stream registered here (the hyperprior side stream, see
# Compressor2018) gets its weight / bias gradient as a separate autograd node whose forward, and so
# whose backward, runs on the registered weight-gradient stream:
#     y = Join(ConvData(x, w.detach(), b.detach()), WGrad(x, w, b))
# WGrad is created first, so its sequence number is lower than ConvData's: when Join's gradient
# arrives, the engine runs ConvData's backward (the input gradient, on the side stream) before
# WGrad's (the weight gradient, on its own stream).  The hyperprior's backward chain -- the input
# gradients that g_a's backward waits for -- then no longer queues behind its weight gradients,
# which run beside the rest of the step.  The parameters' AccumulateGrad nodes are made on the
# weight-gradient stream (the parameters enter the graph through WGrad), the end of backward joins
# every leaf stream, and the arithmetic is the unsplit conv's (the same kernels on the same operands).
_WG_STREAMS = {}   # producing stream handle -> the stream its convs' weight gradients run on
_ZERO = {}         # device index -> a zero scalar (WGrad's output is an expanded view of it)


def route_weight_gradients(stream, wstream):
    """Convs run on `stream` compute their weight gradients on `wstream` (see above)."""
    _WG_STREAMS[stream.cuda_stream] = wstream


def _wgrad_stream(x, weight):
    if not _WG_STREAMS or not x.is_cuda or not torch.is_grad_enabled() or not weight.requires_grad:
        return None
    return _WG_STREAMS.get(torch.cuda.current_stream(x.device).cuda_stream)


class _ConvWGradFn(Function):
    """The weight and bias gradient of a conv (WGrad above).  Forward: nothing (an expanded zero of
    the conv output's shape); backward, on the stream the forward ran on: the wgrad kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, holder, conf, shape):
        dev = x.device.index
        if dev not in _ZERO:
            _ZERO[dev] = torch.zeros((), device=x.device, dtype=torch.float32)
        ctx.holder = holder
        ctx.conf = conf
        ctx.has_b = bias is not None
        ctx.save_for_backward(x, weight)
        return _ZERO[dev].expand(shape)

    @staticmethod
    def backward(ctx, gz):
        x, w = ctx.saved_tensors
        transposed, stride, padding, act, math = ctx.conf
        cur = torch.cuda.current_stream(x.device)
        x.record_stream(cur)   # x and the incoming gradient were allocated on the producing stream
        gz.record_stream(cur)
        pre = _take_colsum(gz) if (ctx.has_b and not act) else None  # bias gradient formed by gz's producer
        if pre is not None:
            pre.record_stream(cur)
        if act:
            # the fused-ReLU output was allocated on the producing (side) stream and is read here
            ctx.holder["y"].record_stream(cur)
        gy = relu_bwd(ctx.holder["y"], gz) if act else gz
        gy = _cl(gy)
        op = _CONV_OP[transposed] + "_wgrad"
        dw, db = getattr(_lib.ops(), op)(x, gy, w, stride, padding, ctx.has_b and pre is None, math)
        _log_plan(op, x, gy, w.shape[2], stride, padding, math)
        return None, dw, ((db if pre is None else pre) if ctx.has_b else None), None, None, None


class _JoinFn(Function):
    """y, passing its gradient to both the input-gradient and the weight-gradient node."""

    @staticmethod
    def forward(ctx, y, z):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return g, g


def _deferred_wgrad(ws, data_fn, x, weight, bias, args, conf, shape):
    ws.wait_stream(torch.cuda.current_stream(x.device))
    holder = {}
    with torch.cuda.stream(ws):
        z = _ConvWGradFn.apply(x, weight, bias, holder, conf, shape)
    y = data_fn.apply(x, weight.detach(), None if bias is None else bias.detach(), *args)
    if conf[3]:
        holder["y"] = y
    return _JoinFn.apply(y, z)


def _conv(fn, x, weight, bias, geom, act, math, cout, out):
    """The three ways a conv runs.  fn: Conv2dFn / ConvTranspose2dFn; geom: (stride, padding) and, transposed,
    output_padding; cout and out(n): the output's channels and its height / width from the input's."""
    if _wcache_on(x):
        return _cached_conv(_CONV_OP[fn.transposed] + "_fwd_ws", x, weight, bias, geom + (act,), math)
    ws = _wgrad_stream(x, weight)
    if ws is not None:
        shape = (x.shape[0], cout, out(x.shape[2]), out(x.shape[3]))
        return _deferred_wgrad(ws, fn, x, weight, bias, geom + (act, math),
                               (fn.transposed, geom[0], geom[1], act, math), shape)
    return fn.apply(x, weight, bias, *geom, act, math)


def conv2d(x, weight, bias=None, stride=1, padding=0, act=0, math=0):
    """`math` (forward and input gradient): 0 fp32 (default), 1 bf16 operands with fp32
    accumulation, 2 fp32 by exact bf16 split (see MATH)."""
    k = weight.shape[2]
    return _conv(Conv2dFn, x, weight, bias, (int(stride), int(padding)), int(act), int(math), weight.shape[0],
                 lambda n: (n + 2 * padding - k) // stride + 1)


def conv_transpose2d(x, weight, bias=None, stride=1, padding=0, output_padding=0, act=0, math=0):
    k = weight.shape[2]
    return _conv(ConvTranspose2dFn, x, weight, bias, (int(stride), int(padding), int(output_padding)), int(act),
                 int(math), weight.shape[1], lambda n: (n - 1) * stride - 2 * padding + k + output_padding)


# ============================================================== GDN
_NORM_RECOMPUTE = os.environ.get("IMGCOMP_GDN_NORM_RECOMPUTE", "1") != "0"  # A/B knob (diagnostic)


def _norm_recompute(x, math, math_fwd):
    """Whether GDN leaves norm out of its forward and recomputes it in the backward: bf16 operands in
    both directions at C = 192 (the fused bf16 kernels, config C3)."""
    return bool(_NORM_RECOMPUTE and (int(math) & MATH["bf16"]) and (int(math_fwd) & MATH["bf16"]) and x.dim() == 4
                and x.shape[1] == 192)


class GDNFn(Function):
    """modelling/layers/gdn.py:84-86 given re-parameterised gamma (C,C,1,1), beta (C,)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, inverse, math=0, math_fwd=0, xb=0):
        _lib.require_device(x, gamma, beta)
        x = _cl(x)
        g = gamma.contiguous()
        b = beta.contiguous()
        # xb & 1: y's bf16 copy for the next conv's forward; xb & 2: dx's for the previous
        # transposed conv's input gradient (bf16 operands only; see _put_bf16)
        # (not under the eval weight cache: its convs (_cached_conv) never take the copy)
        copy = bool((xb & 1) and (int(math_fwd) & MATH["bf16"]) and not _wcache_on(x))
        # bf16 operands at C = 192 (config C3): norm is not stored; the backward forms it again from
        # x, gamma and beta, bitwise as the forward did (include/imgcomp.h ic_gdn_fwd_rn, round 6)
        ctx.rn = _norm_recompute(x, math, math_fwd)
        if ctx.rn:
            y, yb = _lib.ops().gdn_fwd_rn(x, g, b, bool(inverse), int(math_fwd), copy)
            norm = b  # saved in norm's place: the backward's beta
        elif copy:
            y, norm, yb = _lib.ops().gdn_fwd_xb(x, g, b, bool(inverse), int(math_fwd))
        else:
            y, norm = _lib.ops().gdn_fwd(x, g, b, bool(inverse), int(math_fwd))
        if copy:
            _put_bf16(y, yb)
        _log_plan("gdn_fwd", x, None, math=math_fwd)
        ctx.inverse = bool(inverse)
        ctx.math = int(math)
        ctx.xb = int(xb)
        ctx.save_for_backward(x, norm, g)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, norm, g = ctx.saved_tensors
        gy = _match(gy, x)
        # dx's column sums come with it (the fused backward forms them from its dx tiles): the
        # bias gradient of the conv that produced x, taken by that conv's backward (_take_colsum)
        copy = bool((ctx.xb & 2) and (ctx.math & MATH["bf16"]))
        if ctx.rn:  # `norm` holds beta here
            dx, dg, dbeta, dxsum, dxb = _lib.ops().gdn_bwd_sum_rn(x, norm, gy, g, ctx.inverse, ctx.math, copy)
            if copy:
                _put_bf16(dx, dxb)
        elif copy:
            dx, dg, dbeta, dxsum, dxb = _lib.ops().gdn_bwd_sum_xb(x, norm, gy, g, ctx.inverse, ctx.math)
            _put_bf16(dx, dxb)
        else:
            dx, dg, dbeta, dxsum = _lib.ops().gdn_bwd_sum(x, norm, gy, g, ctx.inverse, ctx.math)
        _put_colsum(dx, dxsum)
        _log_plan("gdn_bwd", x, None, math=ctx.math)
        return dx, dg, dbeta, None, None, None, None


def gdn(x, gamma, beta, inverse=False, math=0, math_fwd=0, xb=0):
    """`math` 2: the backward's dgamma GEMM in split arithmetic (C = 192); `math_fwd` 2: the
    forward on the split implicit GEMM instead of the fused fp32 kernel; `xb`: bf16 copies of the
    output (1) / input gradient (2) for the neighbouring conv (bf16 operands, see _put_bf16)."""
    return GDNFn.apply(x, gamma, beta, bool(inverse), int(math), int(math_fwd), int(xb))


class NonNegFn(Function):
    """NonNegativeParam.forward (gdn.py:59-62): max(p, bound)^2 - pedestal."""

    @staticmethod
    def forward(ctx, p, bound, pedestal):
        _lib.require_device(p)
        p = p.contiguous()
        out = _lib.ops().nonneg_fwd(p, float(bound), float(pedestal))
        ctx.bound = float(bound)
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return _lib.ops().nonneg_bwd(p, _match(g, p), ctx.bound), None, None


class NonNegMultiFn(Function):
    """NonNegativeParam.forward (gdn.py:59-62) of several parameters in one launch, and their
    gradients in one launch (torch.ops.imgcomp.nonneg_multi_*; bitwise NonNegFn per tensor).
    Compressor2018 applies it to each transform's GDN gamma / beta once per forward: 2 launches per
    transform per step instead of 12 (6 GDN layers x 2 parameters, forward and backward)."""

    @staticmethod
    def forward(ctx, bounds, peds, *params):
        _lib.require_device(*params)
        ps = [p.contiguous() for p in params]
        outs = _lib.ops().nonneg_multi_fwd(ps, [float(b) for b in bounds], [float(q) for q in peds])
        ctx.bounds = [float(b) for b in bounds]
        ctx.save_for_backward(*ps)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        ps = ctx.saved_tensors
        out = [None] * len(ps)
        idx = [i for i, g in enumerate(gs) if g is not None]
        if idx:
            gi = _lib.ops().nonneg_multi_bwd([ps[i] for i in idx], [_match(gs[i], ps[i]) for i in idx],
                                             [ctx.bounds[i] for i in idx])
            for i, g in zip(idx, gi):
                out[i] = g
        return (None, None, *out)


# ============================================================== elementwise
class BoundFn(Function):
    """LowerBound (upper=False) / UpperBound (upper=True), layers/bound.py:28-59."""

    @staticmethod
    def forward(ctx, x, bound, upper):
        _lib.require_device(x)
        x = _dense(x)
        y = _lib.ops().bound_fwd(x, float(bound), bool(upper))
        ctx.conf = (float(bound), bool(upper))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        bound, upper = ctx.conf
        return _lib.ops().bound_bwd(x, _match(g, x), bound, upper), None, None


class ReLUFn(Function):
    @staticmethod
    def forward(ctx, x):
        _lib.require_device(x)
        y = _lib.ops().relu_fwd(_dense(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return relu_bwd(y, g)


def relu_bwd(y, g):
    return _lib.ops().relu_bwd(y, _match(g, y))


class AbsFn(Function):
    @staticmethod
    def forward(ctx, x):
        _lib.require_device(x)
        x = _dense(x)
        ctx.save_for_backward(x)
        return _lib.ops().abs_fwd(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return _lib.ops().abs_bwd(x, _match(g, x))


class ExpClampFn(Function):
    """torch.clamp(v.exp(), lo, hi) of prior_synthesis.py:72."""

    @staticmethod
    def forward(ctx, v, lo, hi):
        _lib.require_device(v)
        s, e = _lib.ops().exp_clamp_fwd(_dense(v), float(lo), float(hi))
        ctx.conf = (float(lo), float(hi))
        ctx.save_for_backward(e)
        return s

    @staticmethod
    def backward(ctx, g):
        (e,) = ctx.saved_tensors
        lo, hi = ctx.conf
        return _lib.ops().exp_clamp_bwd(e, _match(g, e), lo, hi), None, None


# ============================================================== losses
class CELossFn(Function):
    """_ce_loss (entropy_model.py:185): sum clamp(-ln(p+1e-10)/ln 2, 0, 50)."""

    @staticmethod
    def forward(ctx, p):
        _lib.require_device(p)
        p = _dense(p)
        ctx.save_for_backward(p)
        return _lib.ops().ce_loss_fwd(p)

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return _lib.ops().ce_loss_bwd(p, g)


class MSEFn(Function):
    """nn.MSELoss(reduction='mean')(input, target)."""

    @staticmethod
    def forward(ctx, a, b):
        _lib.require_device(a, b)
        a = _dense(a)
        b = _match(b, a)
        ctx.save_for_backward(a, b)
        return _lib.ops().mse_fwd(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga, gb = _lib.ops().mse_bwd(a, b, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (ga if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None)


# ============================================================== entropy models
def _to_last(t):
    """(N, C, *) -> dense (N, *, C) so that channel = flat index % C."""
    return t.movedim(1, -1).contiguous()


def _from_last(t):
    return t.movedim(-1, 1)


def _noise_arg(z, mode, u, last=False):
    """The `u` operand of the quantizers: injected U[0,1) draws (mode 0, laid out like the
    operand), the device Philox state (mode 3) or nothing."""
    if u is None or mode == 3:
        return u
    u = u.to(z.dtype)
    return _to_last(u) if last else _match(u, z)


class FactorizedFn(Function):
    """EntropyModel._quantize + _prob_mass (entropy_model.py:216-269).
    Returns (q, p) in the input's logical (N, C, *) shape."""

    @staticmethod
    def forward(ctx, z, mode, u, seed, offset, *params):
        _lib.require_device(z, None if mode == 3 else u, *params)
        C = z.shape[1]
        zl = _to_last(z)
        prm = [t.contiguous() for t in params]
        q, p = _lib.ops().factorized_fwd(zl, C, prm, int(mode), _noise_arg(zl, mode, u, last=True), int(seed),
                                         int(offset))
        ctx.mode = int(mode)
        ctx.C = C
        ctx.save_for_backward(q, *prm)
        return _from_last(q), _from_last(p)

    @staticmethod
    def backward(ctx, gq, gp):
        q, *prm = ctx.saved_tensors
        gql = None if (gq is None or ctx.mode == 1) else _to_last(gq)
        gpl = None if gp is None else _to_last(gp)
        dz, grads = _lib.ops().factorized_bwd(q, ctx.C, prm, gql, gpl)
        if ctx.mode == 1:  # torch.round has zero gradient
            dz.zero_()
        return (_from_last(dz), None, None, None, None, *grads)


class FactorizedNetFn(Function):
    """EntropyModel with any CDF MLP widths (cfg DIMS) and any BIN (entropy_model.py:88-99,
    :198, :229-232, :259-269) on the generic kernels (torch.ops.imgcomp.factorized_net_*): the
    register kernels up to 5 hidden layers of width <= 8, the wide kernels beyond (up to 31 hidden
    layers of width <= 256)."""

    @staticmethod
    def forward(ctx, z, mode, u, seed, offset, dims, bin_, *params):
        _lib.require_device(z, None if mode == 3 else u, *params)
        if len(dims) - 1 > _lib.FACT_NET_MAXL or max(dims[1:-1] or [1]) > _lib.FACT_WIDE_MAXW:
            raise NotImplementedError(f"CDF MLP dims {list(dims)}: the kernels take <= {_lib.FACT_NET_MAXL} "
                                      f"layers of width <= {_lib.FACT_WIDE_MAXW}")
        C = z.shape[1]
        zl = _to_last(z)
        prm = [t.contiguous() for t in params]
        q, p = _lib.ops().factorized_net_fwd(zl, C, list(dims), float(bin_), prm, int(mode),
                                             _noise_arg(zl, mode, u, last=True), int(seed), int(offset))
        ctx.conf = (int(mode), C, tuple(dims), float(bin_))
        ctx.save_for_backward(q, *prm)
        return _from_last(q), _from_last(p)

    @staticmethod
    def backward(ctx, gq, gp):
        q, *prm = ctx.saved_tensors
        mode, C, dims, bin_ = ctx.conf
        gql = None if (gq is None or mode == 1) else _to_last(gq)
        gpl = None if gp is None else _to_last(gp)
        dz, grads = _lib.ops().factorized_net_bwd(q, C, list(dims), bin_, prm, gql, gpl)
        if mode == 1:  # torch.round has zero gradient
            dz.zero_()
        return (_from_last(dz), None, None, None, None, None, None, *grads)


class ConditionalFn(Function):
    """SymmetricConditionalModel._quantize + _prob_mass (entropy_model.py:319-352)."""

    @staticmethod
    def forward(ctx, y, scale, mean, kind, mode, u, seed, offset, bin_=1.0):
        _lib.require_device(y, scale, mean, None if mode == 3 else u)
        y = _dense(y)
        scale = _match(scale, y)
        if mean is not None:
            mean = _match(mean, y)
        q, p = _lib.ops().conditional_fwd(y, scale, mean, int(kind), int(mode), _noise_arg(y, mode, u), int(seed),
                                          int(offset), float(bin_))
        ctx.conf = (int(kind), int(mode), mean is not None, float(bin_))
        ctx.save_for_backward(q, scale, mean)
        return q, p

    @staticmethod
    def backward(ctx, gq, gp):
        q, scale, mean = ctx.saved_tensors
        kind, mode, has_mean, bin_ = ctx.conf
        gq = None if gq is None else _match(gq, q)
        gp = None if gp is None else _match(gp, q)
        need = ctx.needs_input_grad
        dy, ds, dm = _lib.ops().conditional_bwd(q, scale, mean, kind, bin_, gq, gp, need[0], need[1],
                                                has_mean and need[2])
        dy = dy if need[0] else None
        if mode == 1 and dy is not None:  # round: zero gradient through q
            dy.zero_()
        return (dy, ds if need[1] else None, dm if (has_mean and need[2]) else None,
                None, None, None, None, None, None)


class QuantizeFn(Function):
    """SymmetricConditionalModel._quantize alone (entropy_model.py:319-336): y + (u - bin/2) in
    training (straight-through: dq/dy = 1), round(y) in evaluation (zero gradient).  The same
    draws, element for element, as ConditionalFn's quantization (torch.ops.imgcomp.quantize)."""

    @staticmethod
    def forward(ctx, y, mode, u, seed, offset, bin_):
        _lib.require_device(y, None if mode == 3 else u)
        y = _dense(y)
        q = _lib.ops().quantize(y, int(mode), _noise_arg(y, mode, u), int(seed), int(offset), float(bin_))
        ctx.mode = int(mode)
        return q

    @staticmethod
    def backward(ctx, gq):
        if ctx.mode == 1:  # torch.round has zero gradient
            return torch.zeros_like(gq), None, None, None, None, None
        return gq, None, None, None, None, None


def quantize(y, train, u=None, bin_=1.0):
    """The conditional model's quantization on its own (see conditional_likelihood)."""
    if not train:
        mode, seed, off = 1, 0, 0
    elif u is not None:
        mode, seed, off = 0, 0, 0
    else:
        mode, seed = 3, 0
        u, off = _noise.philox_stream(y.numel(), y.device)
    return QuantizeFn.apply(y, mode, u, seed, off, float(bin_))


def conditional_likelihood(q, scale, mean, kind, bin_=1.0):
    """The conditional model's likelihood of already-quantized symbols q (ConditionalFn mode 4:
    q passes through unchanged, gradients reach q and scale as in the fused op)."""
    return ConditionalFn.apply(q, scale, mean, kind, 4, None, 0, 0, float(bin_))[1]


def factorized(z, params, train, u=None, dims=(1, 3, 3, 3, 1), bin_=1.0):
    """Returns (q, p) for EntropyModel; `u` optional injected U[0,1) draws.  The default CDF MLP
    (DIMS [3, 3, 3]) with BIN 1 runs the fused fixed-width kernels, anything else the generic ones."""
    if not train:
        mode, seed, off = 1, 0, 0
    elif u is not None:
        mode, seed, off = 0, 0, 0
    else:
        mode, seed = 3, 0
        u, off = _noise.philox_stream(z.numel(), z.device)
    if list(dims) == [1, 3, 3, 3, 1] and float(bin_) == 1.0:
        return FactorizedFn.apply(z, mode, u, seed, off, *params)
    return FactorizedNetFn.apply(z, mode, u, seed, off, tuple(int(d) for d in dims), float(bin_), *params)


def conditional(y, scale, mean, kind, train, u=None, bin_=1.0):
    if not train:
        mode, seed, off = 1, 0, 0
    elif u is not None:
        mode, seed, off = 0, 0, 0
    else:
        mode, seed = 3, 0
        u, off = _noise.philox_stream(y.numel(), y.device)
    return ConditionalFn.apply(y, scale, mean, kind, mode, u, seed, off, float(bin_))


# ============================================================== checkerboard context model
CKBD_LOG_SCALE_LIMIT = 4.0   # IC_CKBD_LOG_SCALE_LIMIT (csrc/common.h): the clamp of the context's log-scale correction


def _ckbd_last(t):
    """(N, C, H, W) -> the contiguous (N, H, W, C) tensor the checkerboard ops index (no copy when channels-last)."""
    if t.dim() != 4:
        raise ValueError(f"the checkerboard ops take (N, C, H, W) tensors, got {tuple(t.shape)}")
    return _to_last(t)


def _ckbd_pair(ref, *ts):
    _lib.require_device(ref, *ts)
    for t in ts:
        if tuple(t.shape) != tuple(ref.shape):
            raise ValueError(f"checkerboard operands must share one shape, got {tuple(ref.shape)} and {tuple(t.shape)}")
    return [_ckbd_last(t) for t in (ref, *ts)]


class CkbdInputFn(Function):
    """(u, v) = (y, |y - mu|) at the anchors (positions with i + j even), +0.0 elsewhere: the inputs of the
    context convs (torch.ops.imgcomp_ckbd.input_fwd / input_bwd)."""

    @staticmethod
    def forward(ctx, y, mu):
        yl, ml = _ckbd_pair(y, mu)
        ctx.save_for_backward(yl, ml)
        u, v = _lib.ckbd_ops().input_fwd(yl, ml)
        return _from_last(u), _from_last(v)

    @staticmethod
    def backward(ctx, gu, gv):
        yl, ml = ctx.saved_tensors
        gu = torch.zeros_like(yl) if gu is None else _ckbd_last(gu)
        gv = torch.zeros_like(yl) if gv is None else _ckbd_last(gv)
        dy, dmu = _lib.ckbd_ops().input_bwd(yl, ml, gu, gv)
        return _from_last(dy), _from_last(dmu)


class CkbdParamsFn(Function):
    """(mu, sigma) = (mu_h + a, sigma_h * exp(clamp(b, -L, L))) at the non-anchors, (mu_h, sigma_h) bit for bit
    at the anchors, L = CKBD_LOG_SCALE_LIMIT (torch.ops.imgcomp_ckbd.params_fwd / params_bwd)."""

    @staticmethod
    def forward(ctx, mu_h, sigma_h, a, b):
        ml, sl, al, bl = _ckbd_pair(mu_h, sigma_h, a, b)
        ctx.save_for_backward(sl, bl)
        mu, sigma = _lib.ckbd_ops().params_fwd(ml, sl, al, bl)
        return _from_last(mu), _from_last(sigma)

    @staticmethod
    def backward(ctx, gmu, gsigma):
        sl, bl = ctx.saved_tensors
        gmu = torch.zeros_like(sl) if gmu is None else _ckbd_last(gmu)
        gsigma = torch.zeros_like(sl) if gsigma is None else _ckbd_last(gsigma)
        dmu_h, dsigma_h, da, db = _lib.ckbd_ops().params_bwd(sl, bl, gmu, gsigma)
        return _from_last(dmu_h), _from_last(dsigma_h), _from_last(da), _from_last(db)


def ckbd_input(y, mu):
    """The context convs' inputs (u, v) from the quantised latent and the hyperprior's mean (CkbdInputFn)."""
    return CkbdInputFn.apply(y, mu)


def ckbd_params(mu_h, sigma_h, a, b):
    """(mu, sigma): the hyperprior's parameters with the context's corrections at the non-anchors (CkbdParamsFn)."""
    return CkbdParamsFn.apply(mu_h, sigma_h, a, b)


def ckbd_context(y_in, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale):
    """(mu, sigma) of every position from the hyperprior's (mu_h, sigma_h), the anchors of y_in and the two context
    convs' weights (C, C, 5, 5) and biases, by the one batch-invariant kernel (torch.ops.imgcomp_ctx.context_fwd,
    csrc/ckbd_context.hip): `ckbd_params(mu_h, sigma_h, conv(u), conv(v))` of `(u, v) = ckbd_input(y_in, mu_h)`
    computing the 12 live taps at the non-anchors only, in exact fp32, image n's result independent of the batch.
    Inference only: no autograd node.  Inside `weight_cache()` the repacked taps are kept per (weights, versions)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (y_in, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale)):
        raise RuntimeError("ckbd_context has no backward: call it under torch.no_grad() (training runs the context convs)")
    yl, ml, sl = _ckbd_pair(y_in, mu_h, sigma_h)
    _lib.require_device(w_mean, b_mean, w_scale, b_scale)
    ws_ = [t.detach().contiguous() for t in (w_mean, b_mean, w_scale, b_scale)]
    if _wcache_on(w_mean):
        # one entry per mean weight; the scale weight it was packed with is part of its validity
        e, hit = _wcache_get("context", w_mean, (int(w_mean.shape[0]),))
        other = e.get("other")
        hit = hit and other is not None and other[0]() is w_scale and other[1] == w_scale._version
        e["other"] = (weakref.ref(w_scale), w_scale._version)
        if "ws" not in e:
            e["ws"] = torch.empty(16, dtype=torch.uint8, device=yl.device)
        packed = hit and e.get("packed", False)
        mu, sigma = _lib.ctx_ops().context_fwd_ws(yl, ml, sl, *ws_, e["ws"], bool(packed))
        e["packed"] = packed or yl.shape[1] * yl.shape[2] > 1   # a 1 x 1 map has no non-anchor: nothing is packed for it
    else:
        mu, sigma = _lib.ctx_ops().context_fwd(yl, ml, sl, *ws_)
    return _from_last(mu), _from_last(sigma)


# ============================================================== h_s as batch-invariant layers
HS_EPILOGUES = {"none": 0, "relu": 1, "exp_clamp": 2}   # IC_HS_NONE / IC_HS_RELU / IC_HS_EXP_CLAMP (include/imgcomp.h)
HS_MAX_KERNEL, HS_STRIDES, HS_MAX_CHANNELS = 5, (1, 2), 4096   # what csrc/hs_invariant.hip serves (k odd)
HS_SIGMA_CLAMP = (1e-10, 1e10)   # h_s's clamp of exp(.) (prior_synthesis.py), the exp_clamp epilogue's default


def hs_supported(cin, cout, k, stride):
    """Whether `hs_layer` serves ConvTranspose2d(cin, cout, k, stride, padding=k // 2, output_padding=stride - 1)."""
    return (1 <= int(cin) <= HS_MAX_CHANNELS and 1 <= int(cout) <= HS_MAX_CHANNELS and int(k) % 2 == 1
            and 1 <= int(k) <= HS_MAX_KERNEL and int(stride) in HS_STRIDES)


def hs_layer(x, weight, bias, stride, epilogue, second=None, clamp=HS_SIGMA_CLAMP):
    """One layer of h_s by the batch-invariant kernel (torch.ops.imgcomp_hs.layer, csrc/hs_invariant.hip):
    `conv_transpose2d(x, weight, bias, stride, padding=k // 2, output_padding=stride - 1)` followed by `epilogue`
    ("none", "relu", or "exp_clamp": clamp(exp(.), *clamp)), in exact fp32, on the logical (N, C, H, W) view of
    channels-last storage.  `second` = (weight, bias, epilogue): a second head on the same input in the same launch;
    the result is then a pair.  Every output's bits depend on the values its taps see, the weights and
    (k, stride, Cin) only -- not on the batch, the map's size or the position's place in it (the order: codec.py).
    Inference only: no autograd node.  Inside `weight_cache()` the repacked taps are kept per (weights, versions)."""
    heads = [(weight, bias, epilogue)] + ([tuple(second)] if second is not None else [])
    params = [t for w, b, _ in heads for t in (w, b)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, *params)):
        raise RuntimeError("hs_layer has no backward: call it under torch.no_grad() (training runs the convs)")
    for _, _, e in heads:
        if e not in HS_EPILOGUES:
            raise ValueError(f"hs_layer: no epilogue {e!r} (one of {sorted(HS_EPILOGUES)})")
    _lib.require_device(x, *params)
    xl = _ckbd_last(x)
    ps = [t.detach().contiguous() for t in params]
    w2, b2 = (ps[2], ps[3]) if second is not None else (None, None)
    args = (xl, ps[0], ps[1], int(stride), HS_EPILOGUES[epilogue], w2, b2,
            HS_EPILOGUES[heads[-1][2]] if second is not None else 0, float(clamp[0]), float(clamp[1]))
    if _wcache_on(weight):
        # one entry per first weight; the second head's weight it was packed with is part of its validity
        e, hit = _wcache_get("hs", weight, (tuple(weight.shape), int(stride), len(heads)))
        if second is not None:
            other = e.get("other")
            hit = hit and other is not None and other[0]() is second[0] and other[1] == second[0]._version
            e["other"] = (weakref.ref(second[0]), second[0]._version)
        if "ws" not in e:
            e["ws"] = torch.empty(16, dtype=torch.uint8, device=xl.device)
        packed = hit and e.get("packed", False)
        out, out2 = _lib.hs_ops().layer_ws(*args, e["ws"], bool(packed))
        e["packed"] = True
    else:
        out, out2 = _lib.hs_ops().layer(*args)
    return _from_last(out) if second is None else (_from_last(out), _from_last(out2))


# ============================================================== gain units
class GainVectorFn(Function):
    """(len(q), C) gain vectors of the level table (S, C) at the qualities q (a tuple of floats in [0, S-1]): the
    gain-vector rule of codec.py (torch.ops.imgcomp_gain.gain_vector / gain_vector_bwd)."""

    @staticmethod
    def forward(ctx, table, q):
        _lib.require_device(table)
        q = [float(v) for v in q]
        g = _lib.gain_ops().gain_vector(table.contiguous(), q)
        ctx.save_for_backward(g)
        ctx.q, ctx.levels = q, int(table.shape[0])
        return g

    @staticmethod
    def backward(ctx, dg):
        g, = ctx.saved_tensors
        return _lib.gain_ops().gain_vector_bwd(g, dg.contiguous(), ctx.levels, ctx.q), None


class ChannelScaleFn(Function):
    """x (N, C, *) times the gains g (1 or N, C), row 0 for every image or row n for image n: one fp32
    multiplication per element (torch.ops.imgcomp_gain.channel_scale / channel_scale_bwd)."""

    @staticmethod
    def forward(ctx, x, g):
        _lib.require_device(x, g)
        if x.dim() < 2 or g.dim() != 2 or g.shape[1] != x.shape[1] or g.shape[0] not in (1, x.shape[0]):
            raise ValueError(f"the gains {tuple(g.shape)} must be (1 or N, C) for a tensor of shape {tuple(x.shape)}")
        xl, g = _to_last(x), g.contiguous()
        ctx.save_for_backward(xl, g)
        return _from_last(_lib.gain_ops().channel_scale(xl, g))

    @staticmethod
    def backward(ctx, dy):
        xl, g = ctx.saved_tensors
        dx, dg = _lib.gain_ops().channel_scale_bwd(xl, g, _to_last(dy))
        return _from_last(dx), dg


def gain_vector(table, q):
    """The gain vectors (len(q), C) of a level table at the qualities q (GainVectorFn)."""
    return GainVectorFn.apply(table, tuple(q))


def channel_scale(x, g):
    """x (N, C, *) scaled per channel by the gains g (1 or N, C) (ChannelScaleFn)."""
    return ChannelScaleFn.apply(x, g)


# ============================================================== coding to a byte budget
def _on_device(who, **operands):
    for what, t in operands.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"imgcomp: HIP kernels need tensors on a ROCm (cuda) device; {who} got {what} on {t.device}")


def measure_seg(sym, nseg, rows, channels, pool, nrows, seg_k, seg_off, steps_per_chunk):
    """The chunk lengths the segmented coder reports for these symbols and tables, int32 (nseg * chunks per segment)
    on the device, without coding a byte: the operands of torch.ops.imgcomp_stream.encode_seg
    (torch.ops.imgcomp_rate.measure_seg).  Inference only."""
    _on_device("measure_seg", sym=sym, rows=rows, pool=pool)
    return _lib.rate_ops().measure_seg(sym, int(nseg), rows, int(channels), pool, int(nrows), [int(k) for k in seg_k],
                                       [int(o) for o in seg_off], int(steps_per_chunk))


def gain_symbolize_seg(y, g, mean, img):
    """The symbols of y (N, C, *) for M candidates: candidate m is image img[m] scaled by the gain row g[m] of g
    (M, C) and coded about mean[m] of mean (M, C, *) -> (int32 rint(y[img[m]] * g[m] - mean[m]) of the M candidates
    back to back, each in (*, c) order, [kmax of candidate m]).  Bit for bit `channel_scale` then
    `symbolize_mean_seg` on the gathered batch y[img], which is never formed
    (torch.ops.imgcomp_rate.gain_symbolize_seg).  Inference only; ValueError naming the candidate whose symbols
    exceed the coder's limit."""
    _lib.require_device(y, g, mean)
    img = [int(i) for i in img]
    if y.dim() < 2 or g.dim() != 2 or tuple(g.shape) != (len(img), y.shape[1]):
        raise ValueError(f"the gains {tuple(g.shape)} must be ({len(img)} candidates, C) for a tensor of shape "
                         f"{tuple(y.shape)}")
    if tuple(mean.shape) != (len(img), *y.shape[1:]):
        raise ValueError(f"the mean {tuple(mean.shape)} must hold {len(img)} candidates of shape {tuple(y.shape[1:])}")
    _inference_only("gain_symbolize_seg", y=y, g=g, mean=mean)
    sym, kmax = _lib.rate_ops().gain_symbolize_seg(_to_last(y.detach()), g.detach().contiguous(), _to_last(mean.detach()),
                                                   img)
    return sym, [int(k) for k in kmax]


# ============================================================== transcoding in the latent domain
def requant_seg(r, mu1, a, b, mu2, img):
    """The symbols of y at M target qualities from N decoded streams: r (N, C, *) the decoder's float integers of y,
    mu1 (N, C, *) their means, a (N, C) the sources' inverse gains; target m is source img[m] under the gain row b[m]
    of b (M, C), coded about mu2[m] of mu2 (M, C, *) -> (int32 rint(((r + mu1) * a) * b - mu2) of the M targets back
    to back, each in (*, c) order, [kmax of target m]), every operation one fp32 operation.  Bit for bit `add_mean`,
    `channel_scale` twice and `symbolize_mean_seg` on the gathered batch, which is never formed
    (torch.ops.imgcomp_transcode.requant_seg; the requantization rule of codec.py).  Inference only; ValueError naming
    the target whose symbols exceed the coder's limit."""
    _lib.require_device(r, mu1, a, b, mu2)
    img = [int(i) for i in img]
    if r.dim() < 2 or tuple(mu1.shape) != tuple(r.shape):
        raise ValueError(f"the mean {tuple(mu1.shape)} must have the shape of the integers {tuple(r.shape)}")
    if a.dim() != 2 or tuple(a.shape) != (r.shape[0], r.shape[1]):
        raise ValueError(f"the source gains {tuple(a.shape)} must be ({r.shape[0]} sources, C) for a tensor of shape "
                         f"{tuple(r.shape)}")
    if b.dim() != 2 or tuple(b.shape) != (len(img), r.shape[1]):
        raise ValueError(f"the target gains {tuple(b.shape)} must be ({len(img)} targets, C) for a tensor of shape "
                         f"{tuple(r.shape)}")
    if tuple(mu2.shape) != (len(img), *r.shape[1:]):
        raise ValueError(f"the mean {tuple(mu2.shape)} must hold {len(img)} targets of shape {tuple(r.shape[1:])}")
    _inference_only("requant_seg", r=r, mu1=mu1, a=a, b=b, mu2=mu2)
    sym, kmax = _lib.transcode_ops().requant_seg(_to_last(r.detach()), _to_last(mu1.detach()), a.detach().contiguous(),
                                                 b.detach().contiguous(), _to_last(mu2.detach()), img)
    return sym, [int(k) for k in kmax]


# ============================================================== region-of-interest coding
def _block_map(idx, device):
    """A block map as the kernels take it: contiguous uint8 on the device."""
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.uint8 or idx.dim() != 3:
        raise ValueError("a block map is a uint8 tensor (N, blocks down, blocks across)")
    if not idx.is_cuda:
        raise RuntimeError(f"imgcomp: HIP kernels need tensors on a ROCm (cuda) device; got a block map on {idx.device}")
    return idx.contiguous()


class BlockScaleFn(Function):
    """x (N, C, H, W) times row idx[n, i >> shift, j >> shift] of the gains g (R, C) at position (i, j): one fp32
    multiplication per element (torch.ops.imgcomp_region.block_scale / block_scale_bwd)."""

    @staticmethod
    def forward(ctx, x, g, idx, shift):
        _lib.require_device(x, g)
        shift = int(shift)
        if x.dim() != 4 or g.dim() != 2 or g.shape[1] != x.shape[1] or not 1 <= g.shape[0] <= 256:
            raise ValueError(f"the gains {tuple(g.shape)} must be (1 .. 256, C) for a tensor of shape {tuple(x.shape)}")
        if not 0 <= shift <= 6:
            raise ValueError(f"a block is 2^shift positions wide, shift in 0 .. 6, got {shift}")
        idx = _block_map(idx, x.device)
        want = (x.shape[0], -(-x.shape[2] >> shift), -(-x.shape[3] >> shift))
        if tuple(idx.shape) != want:
            raise ValueError(f"the block map {tuple(idx.shape)} must be {want} for a tensor of shape {tuple(x.shape)} at "
                             f"shift {shift}")
        xl, g = _to_last(x), g.contiguous()
        ctx.save_for_backward(xl, g, idx)
        ctx.shift = shift
        return _from_last(_lib.region_ops().block_scale(xl, g, idx, shift))

    @staticmethod
    def backward(ctx, dy):
        xl, g, idx = ctx.saved_tensors
        dx, dg = _lib.region_ops().block_scale_bwd(xl, g, idx, _to_last(dy), ctx.shift)
        return _from_last(dx), dg, None, None


class BlockMSEFn(Function):
    """(the mean of w[idx[n, i >> 6, j >> 6]] (a - b)^2, the plain mean of (a - b)^2) of two images (N, C, H, W), from
    one pass; the second carries no gradient (torch.ops.imgcomp_region.block_mse_fwd / block_mse_bwd)."""

    @staticmethod
    def forward(ctx, a, b, w, idx):
        _lib.require_device(a, b, w)
        if a.dim() != 4 or w.dim() != 1 or not 1 <= w.shape[0] <= 256:
            raise ValueError(f"block_mse takes images (N, C, H, W) and 1 .. 256 weights, got {tuple(a.shape)} and "
                             f"{tuple(w.shape)}")
        idx = _block_map(idx, a.device)
        want = (a.shape[0], -(-a.shape[2] // 64), -(-a.shape[3] // 64))
        if tuple(idx.shape) != want:
            raise ValueError(f"the block map {tuple(idx.shape)} must be {want} for images of shape {tuple(a.shape)}")
        a = _dense(a)
        b = _match(b, a)
        w = w.contiguous()
        ctx.save_for_backward(a, b, w, idx)
        out = _lib.region_ops().block_mse_fwd(a, b, w, idx)
        weighted, plain = out[0], out[1]
        ctx.mark_non_differentiable(plain)
        return weighted, plain

    @staticmethod
    def backward(ctx, g, _g_plain):
        a, b, w, idx = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        if not any(need):
            return None, None, None, None
        ga, gb = _lib.region_ops().block_mse_bwd(a, b, w, idx, g, need[0], need[1])
        return (ga if need[0] else None), (gb if need[1] else None), None, None


def block_scale(x, g, idx, shift):
    """x (N, C, H, W) scaled per channel by the row of g (R, C) its block names: idx uint8 (N, ceil(H / 2^shift),
    ceil(W / 2^shift)) on the device (BlockScaleFn)."""
    return BlockScaleFn.apply(x, g, idx, shift)


def block_mse(a, b, w, idx):
    """(block-weighted mean squared error, plain mean squared error) of two images: w (R) on the device, idx uint8
    (N, ceil(H / 64), ceil(W / 64)) (BlockMSEFn)."""
    return BlockMSEFn.apply(a, b, w, idx)


# ============================================================== a quality map under a byte budget
def block_allocate(bits, sse, img, w, codes):
    """The per-block level choice of M candidates by the allocation rule of codec.py: bits, sse (N, L, nb) the fp32
    tables of N images at L levels; candidate m is image img[m] at the weight w[m] (finite, >= 0, a float32 value);
    codes: the code of every level -> (ranks uint8 (M, nb): the chosen level of every block, codes uint8 (M, nb): its
    code, sums float64 (2, M): the chosen bits and the chosen sse of every candidate, in a fixed order).  On the
    device, no copy to the host (torch.ops.imgcomp_alloc.block_allocate).  Inference only."""
    _lib.require_device(bits, sse)
    _inference_only("block_allocate", bits=bits, sse=sse)
    return _lib.alloc_ops().block_allocate(bits.detach().contiguous(), sse.detach().contiguous(), [int(i) for i in img],
                                           [float(v) for v in w], [int(k) for k in codes])


def block_gain_symbolize_seg(y, g, rank, mean, img, shift=2):
    """`gain_symbolize_seg` with a gain row per block: candidate m is image img[m] of y (N, C, H, W), position (i, j)
    scaled by the row rank[m, i >> shift, j >> shift] of g (R, C) and coded about mean[m] of mean (M, C, H, W); rank is
    uint8 (M, ceil(H / 2^shift), ceil(W / 2^shift)) on the device -> (int32 symbols of the M candidates back to back,
    each in (i, j, c) order, [kmax of candidate m]).  Bit for bit `block_scale` then `symbolize_mean_seg` on the
    gathered batch y[img], which is never formed (torch.ops.imgcomp_alloc.block_gain_symbolize_seg).  Inference only;
    ValueError naming the candidate whose symbols exceed the coder's limit."""
    _lib.require_device(y, g, mean)
    img, shift = [int(i) for i in img], int(shift)
    if y.dim() != 4 or g.dim() != 2 or g.shape[1] != y.shape[1] or not 1 <= g.shape[0] <= 256:
        raise ValueError(f"the gains {tuple(g.shape)} must be (1 .. 256, C) for a tensor of shape {tuple(y.shape)}")
    if not 0 <= shift <= 6:
        raise ValueError(f"a block is 2^shift positions wide, shift in 0 .. 6, got {shift}")
    rank = _block_map(rank, y.device)
    want = (len(img), -(-y.shape[2] >> shift), -(-y.shape[3] >> shift))
    if tuple(rank.shape) != want:
        raise ValueError(f"the rank map {tuple(rank.shape)} must be {want} for {len(img)} candidates of a tensor of shape "
                         f"{tuple(y.shape)} at shift {shift}")
    if tuple(mean.shape) != (len(img), *y.shape[1:]):
        raise ValueError(f"the mean {tuple(mean.shape)} must hold {len(img)} candidates of shape {tuple(y.shape[1:])}")
    _inference_only("block_gain_symbolize_seg", y=y, g=g, mean=mean)
    sym, kmax = _lib.alloc_ops().block_gain_symbolize_seg(_to_last(y.detach()), g.detach().contiguous(), rank,
                                                          _to_last(mean.detach()), img, shift)
    return sym, [int(k) for k in kmax]


# ============================================================== rate and distortion maps
def _map_operand(t, who, what):
    """A map kernel's operand: fp32 (N, C, H, W) on the device; every image dense channels-last or dense NCHW storage
    as it comes, a dense copy otherwise."""
    _lib.require_device(t)
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{who}: {what} must be a non-empty (N, C, H, W) tensor, got {tuple(t.shape)}")
    t = t.detach()
    (_, C, H, W), (_, sc, sh, sw) = t.shape, t.stride()
    last = (C == 1 or sc == 1) and (W == 1 or sw == C) and (H == 1 or sh == W * C)
    nchw = (W == 1 or sw == 1) and (H == 1 or sh == W) and (C == 1 or sc == H * W)
    return t if last or nchw else t.contiguous()


def _inference_only(who, **operands):
    """RuntimeError if autograd would have to record the call: the map kernels have no backward."""
    for what, t in operands.items():
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who} is inference only: {what} requires grad; detach it or call under torch.no_grad()")


def _map_shift(shift):
    shift = int(shift)
    if not 0 <= shift <= 6:
        raise ValueError(f"a block is 2^shift positions wide, shift in 0 .. 6, got {shift}")
    return shift


def block_bits(p, shift, add=None):
    """The estimated bits of every block of 2^shift x 2^shift positions of the likelihoods p (N, C, H, W): the sum over
    the block and all channels of clamp(-log2(p + 1e-10), 0, 50), CELossFn's term, as (N, ceil(H / 2^shift),
    ceil(W / 2^shift)); with `add`, a map of that shape, add + that sum (one fp32 addition).  Inference only: no
    autograd node.  Image n's map has the same bits whatever the batch around it
    (torch.ops.imgcomp_map.block_bits)."""
    _inference_only("block_bits", p=p, add=add)
    p, shift = _map_operand(p, "block_bits", "p"), _map_shift(shift)
    if add is not None:
        _lib.require_device(add)
        want = (p.shape[0], -(-p.shape[2] >> shift), -(-p.shape[3] >> shift))
        if tuple(add.shape) != want:
            raise ValueError(f"block_bits: add {tuple(add.shape)} must be the map {want} of p {tuple(p.shape)} at shift "
                             f"{shift}")
        add = add.detach().contiguous()
    return _lib.map_ops().block_bits(p, shift, add)


def block_sse(a, b, shift=6):
    """The squared error of every block of 2^shift x 2^shift pixels of two images (N, C, H, W): the sum of (a - b)^2
    over the block and all channels, as (N, ceil(H / 2^shift), ceil(W / 2^shift)).  Inference only: no autograd node.
    Image n's map has the same bits whatever the batch around it (torch.ops.imgcomp_map.block_sse)."""
    _inference_only("block_sse", a=a, b=b)
    a, b = _map_operand(a, "block_sse", "a"), _map_operand(b, "block_sse", "b")
    if a.shape != b.shape:
        raise ValueError(f"block_sse: the two images must share a shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _lib.map_ops().block_sse(a, b, _map_shift(shift))


# ============================================================== encode-time latent refinement
# Thin wrappers of torch.ops.imgcomp_refine (csrc/refine.hip): the bookkeeping of Compressor2018.compress_each_refined.
# Inference only, on the current stream; none of them copies to the host or waits for the stream.
class RoundThroughFn(Function):
    """y_hat, the value of `refine_update`'s Evaluate rule at v, as a function of v whose gradient passes straight
    through the rounding to v."""

    @staticmethod
    def forward(ctx, v, y_hat):
        return y_hat.view_as(y_hat)

    @staticmethod
    def backward(ctx, g):
        return g, None


def refine_update(v, m, u, g, mu, lr=0.0, c1=1.0, c2=1.0):
    """One pass over the latent v (N, *, C), contiguous channels-last storage.  With a gradient g: the Adam step on v and
    its moments m, u, all three in place, at the learning rate lr with the bias corrections c1 = 1 / (1 - 0.9^t) and
    c2 = 1 / (1 - 0.999^t) (the fp32 operation order: csrc/refine.hip).  Then, with or without a step, the Evaluate
    rule on v -> (int32 symbols rint(v - mu) flattened, y_hat = symbols + mu shaped like v); mu None: about 0."""
    _on_device("refine_update", v=v, m=m, u=u, g=g, mu=mu)
    _inference_only("refine_update", v=v, m=m, u=u, g=g, mu=mu)
    return _lib.refine_ops().update(v, m, u, g, mu, float(lr), float(c1), float(c2))


def refine_dist_grad(x, x_hat, w):
    """(float32)(2 w[n]) * (x_hat - x): the gradient at x_hat of sum_n w[n] D_n, D_n the squared error of image n;
    x, x_hat contiguous (N, *), w float64 (N) on the device."""
    _on_device("refine_dist_grad", x=x, x_hat=x_hat, w=w)
    return _lib.refine_ops().dist_grad(x.detach(), x_hat.detach(), w)


def refine_objective(bits, sse, w):
    """float64 (3, N): B_n and D_n, the sums of image n's values of the maps `block_bits` / `block_sse` made (both
    (N, Hb, Wb)) in ascending block order in fp64, and J_n = B_n + w[n] D_n; w float64 (N) on the device."""
    _on_device("refine_objective", bits=bits, sse=sse, w=w)
    return _lib.refine_ops().objective(bits, sse, w)


def refine_keep(sym, best_sym, obj, best, best_step, step):
    """Keep-best, image by image: where obj[2, n] < best[2, n] (strict; a NaN never wins) image n's segment of `sym`
    replaces that of `best_sym`, best[:, n] = obj[:, n] and best_step[n] = step; everything else is left alone.  Two
    launches: the symbols, then the scalars the comparison reads."""
    _on_device("refine_keep", sym=sym, best_sym=best_sym, obj=obj, best=best, best_step=best_step)
    _lib.refine_ops().keep(sym, best_sym, obj, best, best_step, int(step))


def refine_kmax(sym, nseg):
    """int32 (nseg) on the device: max |symbol| of each of the nseg equal segments of `sym`."""
    _on_device("refine_kmax", sym=sym)
    return _lib.refine_ops().kmax(sym, int(nseg))


class SqDiffFn(Function):
    """(a - b)^2 elementwise: nn.MSELoss(reduction='none')."""

    @staticmethod
    def forward(ctx, a, b):
        _lib.require_device(a, b)
        a = _dense(a)
        b = _match(b, a)
        ctx.save_for_backward(a, b)
        return _lib.ops().sqdiff_fwd(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga, gb = _lib.ops().sqdiff_bwd(a, b, _match(g, a), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (ga if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None)


class MSSSIMFn(Function):
    """SSIM / MS-SSIM loss (modelling/loss.py:48-188)."""

    @staticmethod
    def forward(ctx, a, b, conf):
        _lib.require_device(a, b)
        (nlev, fs, sigma, max_val, log_scale, single, k1, k2, eps, weights) = conf
        out, state = _lib.ops().msssim_fwd(a, b, nlev, fs, sigma, max_val, bool(log_scale), int(single), k1, k2, eps,
                                           list(weights))
        ctx.conf = conf
        ctx.shape = tuple(a.shape)
        ctx.save_for_backward(state)
        return out

    @staticmethod
    def backward(ctx, g):
        (state,) = ctx.saved_tensors
        (nlev, fs, sigma, max_val, log_scale, single, k1, k2, eps, weights) = ctx.conf
        need = ctx.needs_input_grad
        ga, gb = _lib.ops().msssim_bwd(g, state, list(ctx.shape), nlev, fs, sigma, max_val, bool(log_scale),
                                       int(single), k1, k2, eps, list(weights), need[0], need[1])
        return (ga if need[0] else None), (gb if need[1] else None), None


def msssim(img1, img2, mod, weights, single_scale):
    conf = (len(weights), int(mod.filter_size), float(mod.filter_sigma), float(mod.max_val), bool(mod.log_scale),
            bool(single_scale), float(mod.k1), float(mod.k2), float(mod.eps), [float(w) for w in weights])
    return MSSSIMFn.apply(img1, img2, conf)
