"""autograd glue: every differentiable step of the hot path is a ``torch.autograd.Function`` whose
forward/backward only enqueue kernels of ``libbdvcil_hip.so`` (through ``kernels``).

Granularity is chosen so that no gradient junction inside a residual block is left to autograd
(the identity-path add and its ReLU mask are fused into the conv1 dgrad epilogue):

* ``StemFn``      NHWC4 frames -> conv7x7/2 + BN + ReLU + maxpool3x3/2
* ``ResBlockFn``  one BasicBlock / Bottleneck incl. temporal shift, BN, ReLU, residual
* ``AvgPoolFn``, ``DropoutFn``, ``LSCFn``, ``LinearFn``, ``ConsensusFn``
* ``LSCLossFn``, ``SoftCEFn``, ``KDMSEFn``

Internal activation layout is NHWC fp32; module boundaries expose NCHW *views* of the same
storage (``nhwc_to_nchw_view``), so hooks and feature-distillation see mmaction-shaped tensors.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from . import kernels as K


# ---------------------------------------------------------------------------------------------
# side stream for weight gradients
# ---------------------------------------------------------------------------------------------
# In backward, wgrad(l) only feeds the optimizer while BatchNorm-backward(l) -> dgrad(l) -> BatchNorm-backward(l-1) -> ... is the
# critical chain.  The wgrads are launched on a second HIP stream: the HBM-bound BatchNorm-backward passes of the chain then
# run beside the MFMA-bound wgrad of the layer above (the 8-wave conv kernels occupy one workgroup per CU and leave wave
# slots free), and the CUs a dgrad's last partial round of workgroups leaves idle are filled by wgrad workgroups.
# ``join_side_stream`` must run before gradients are consumed (FusedSGD.step / clip / GradAllReducer / StemFn.backward do it).
# Measured on one box, alternating runs (profiles/r02_side_stream.txt): 535.1 / 535.0 clips/s without, 551.5 / 550.5 with.
# BDVCIL_WGRAD_SIDE_STREAM=0 puts everything back on one stream (one batched split-K reduction per stage then).
import collections as _collections
import os as _os
_SIDE = {'enabled': _os.environ.get('BDVCIL_WGRAD_SIDE_STREAM', '1') != '0', 'streams': {}, 'pending': {}, 'held': {}}
# Lifetime of the operands of a weight gradient running on the side stream.  torch's record_stream() defers the release of a
# block until the side stream's work at release time has finished; the host enqueues a whole step ahead of the device, so none of
# those blocks was ever reusable inside a step and the caching allocator went back to hipMalloc for every gradient and
# activation tensor: 115 GB reserved for 24 GB allocated at batch 32, 225 GB for 46 GB at batch 64 -- where steps then ran
# 1.3 - 2.5 x slower in some processes (gpurun_out/lag*.log: 94 ms against 70 ms per step).  Instead the operands stay referenced
# in a FIFO until the main stream has waited for the side stream (join_side_stream: the end of the backward pass, or a gradient
# bucket becoming ready), after which they return to the pool in plain stream order: 46 GB reserved at batch 32, no extra
# synchronisation, step time level or better (profiles/r02_ab_streams.txt).  BDVCIL_SIDE_LAG bounds the FIFO: the main stream
# waits for the weight gradient that many launches back before dropping its operands (64 = never inside a ResNet-50 step;
# smaller values trade 1 % of step time for a few GB); 0 = record_stream().
SIDE_LAG = int(_os.environ.get('BDVCIL_SIDE_LAG', '64'))


# BatchNorm-backward statistics of a unit taken in the epilogue of the dgrad that produces its output gradient
# (bdv_conv_dgrad with a bdv_bn_stat_fuse): removes the separate pass over dout, y and the mask for the inner units.
FUSE_BN_STATS = _os.environ.get('BDVCIL_FUSE_BN_STATS', '1') != '0'
# A unit's BatchNorm + ReLU applied in the loaders of the conv that consumes it (fprop and weight gradient) instead of in an apply
# pass of its own: conv1 -> conv2 and conv2 -> conv3 inside a block (the block output is read by two consumers and stays a pass).
# The activation and its ReLU mask are then never written; the backward kernels derive the sign from the conv output.
PRE_BN = _os.environ.get('BDVCIL_PRE_BN', '0') == '1'      # off: measured 0.6 ms per step SLOWER; saves ~2.8 GB
# A whole stage as one autograd node (ResStageFn): lets the statistics fusion above reach the block outputs.
FUSE_STAGE = _os.environ.get('BDVCIL_FUSE_STAGE', '1') != '0'
# one split-K reduction launch per autograd node (stage / block) instead of one per conv
BATCH_WGRAD_REDUCE = _os.environ.get('BDVCIL_BATCH_WGRAD_REDUCE', '1') != '0'


# Test hook: when set to a list, every training-mode forward appends the 1-bit ReLU masks it writes, in execution order
# (stem, then per block: unit 0, unit 1, ..., block output); the parity tests compare them with the CPU reference's signs.
RELU_MASK_TAP = None
POOL_IDX_TAP = None      # tests: the stem max-pool's arg-max codes (3 r + s per output element), same purpose


def _tap_mask(shape, mask):
    """Hand one ReLU's sign bits to RELU_MASK_TAP; ``mask`` may be a callable that produces them (run only while the tap is set)."""
    if RELU_MASK_TAP is not None:
        RELU_MASK_TAP.append((tuple(shape), mask() if callable(mask) else mask))


def _tap_pool(idx):
    if POOL_IDX_TAP is not None:
        POOL_IDX_TAP.append(idx)


def set_side_stream_enabled(flag: bool):
    _SIDE['enabled'] = bool(flag)


def side_stream_enabled() -> bool:
    return _SIDE['enabled']


def side_stream(device) -> torch.cuda.Stream:
    return _side_stream(device)[1]


def _side_stream(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _SIDE['streams'].get(idx)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _SIDE['streams'][idx] = st
    return idx, st


def join_side_stream(device=None):
    """Make the current stream wait for every wgrad launched on the side stream so far."""
    for idx, ev in list(_SIDE['pending'].items()):
        if device is None or (device.index if device.index is not None else torch.cuda.current_device()) == idx:
            torch.cuda.current_stream(idx).wait_event(ev)
            del _SIDE['pending'][idx]
            held = _SIDE['held'].get(idx)
            if held:
                held.clear()        # the event is the side stream's latest: the current stream is now behind all of its work


class wgrad_batch:
    """Inside ``with wgrad_batch():`` the split-K reductions of all weight gradients are deferred and run as one launch
    when the block ends (a stage's backward: one reduce kernel instead of one per conv).  The returned dw tensors are
    filled at that point, i.e. before the autograd node hands them out."""
    current = None

    def __enter__(self):
        self.items, self.outer = [], wgrad_batch.current
        if BATCH_WGRAD_REDUCE:
            wgrad_batch.current = self
        return self

    def __exit__(self, exc_type, exc, tb):
        wgrad_batch.current = self.outer
        if exc_type is None and self.items:
            if _SIDE['enabled'] and self.items[0][0].is_cuda:     # the partial products were launched on the side stream
                idx, side = _side_stream(self.items[0][0].device)
                with torch.cuda.stream(side):
                    K.wgrad_reduce_batched(self.items)
                    done = torch.cuda.Event()
                    done.record(side)
                _SIDE['pending'][idx] = done
            else:
                K.wgrad_reduce_batched(self.items)
        self.items = []
        return False


# How the weight gradient of a conv gets its activation operand when the producer's apply pass never ran (PRE_BN):
# 'recompute' (default): one bn_apply on the stream the weight gradient runs on (the side stream: an HBM-bound pass beside the
# main chain's MFMA-bound dgrads), then the plain kernel; 'loader': the producer's BatchNorm + ReLU in the weight-gradient kernel's
# own loader (measured slower in the step: that loader already splits both operands).
PRE_BN_WGRAD = _os.environ.get('BDVCIL_PRE_BN_WGRAD', 'recompute')


def wgrad_overlapped(dy: torch.Tensor, inp: torch.Tensor, geom, pre_bn=None) -> torch.Tensor:
    """Weight gradient of one conv: deferred reduction inside a ``wgrad_batch``, otherwise K.conv_wgrad (optionally on the
    side stream)."""
    batch = wgrad_batch.current
    recompute = pre_bn is not None and PRE_BN_WGRAD != 'loader'
    if not _SIDE['enabled']:
        if recompute:
            inp, pre_bn = K.bn_apply(inp, pre_bn[0], pre_bn[1], None, True), None
        if batch is not None:
            slab, dw = K.conv_wgrad_partial(dy, inp, geom, pre_bn=pre_bn)
            batch.items.append((slab, dw))
            return dw
        return K.conv_wgrad(dy, inp, geom, pre_bn=pre_bn)
    main = torch.cuda.current_stream(dy.device)
    idx, side = _side_stream(dy.device)
    dw = torch.empty((geom.Cout, geom.R, geom.S, geom.Cin), dtype=torch.float32, device=dy.device)   # owned by main
    if not recompute:               # 'f16x2': the operands' amax words are taken here, on the main stream -- the data gradient that
        K.wgrad_amax(dy, inp, geom)  # follows reads dy's too and must not wait for the side stream's queue
    ready = torch.cuda.Event()
    ready.record(main)
    side.wait_event(ready)
    raw = inp                       # what the side stream READS (allocated on main): held / registered below, also when `inp` is rebound
    with torch.cuda.stream(side):
        if recompute:               # the activation exists only for the duration of this weight gradient
            inp = K.bn_apply(inp, pre_bn[0], pre_bn[1], None, True)
            pre_bn = None
        if batch is not None:       # split-K slabs now, one reduction launch (on the side stream) when the stage ends
            slab, _ = K.conv_wgrad_partial(dy, inp, geom, dw=dw, pre_bn=pre_bn)
            batch.items.append((slab, dw))
        else:
            K.conv_wgrad(dy, inp, geom, dw=dw, beta=0.0, ws_tag='wgrad_side', pre_bn=pre_bn)
        done = torch.cuda.Event()
        done.record(side)
    if SIDE_LAG > 0:
        held = _SIDE['held'].setdefault(idx, _collections.deque())
        held.append((done, (dy, raw, inp)))
        while len(held) > SIDE_LAG:
            ev, _ = held.popleft()
            main.wait_event(ev)     # (long finished: the side stream runs beside the main chain, not behind it)
    else:
        for t in (dy, raw, inp, dw):
            t.record_stream(side)
    _SIDE['pending'][idx] = done
    return dw


# The downsample branch of a block (1x1 conv + its BatchNorm statistics) depends only on the block input: it can run on the
# side stream beside conv1 / conv2 / conv3 of the main branch and is joined before the block-output kernel.
DS_SIDE = _os.environ.get('BDVCIL_DS_SIDE', '1') != '0'


def run_on_side_stream(fn, device):
    """Run ``fn()`` (kernel launches only) on the side stream after everything enqueued on the current stream so far;
    returns (result, event).  The caller makes the consumer stream wait for the event; tensors created inside are
    registered with the current stream as well, so their memory is not recycled under the consumer."""
    main = torch.cuda.current_stream(device)
    _, side = _side_stream(device)
    ready = torch.cuda.Event()
    ready.record(main)
    side.wait_event(ready)
    with torch.cuda.stream(side):
        K.WS_TAG_SUFFIX = '_side'
        try:
            out = fn()
        finally:
            K.WS_TAG_SUFFIX = ''
        done = torch.cuda.Event()
        done.record(side)
    for t in (out if isinstance(out, (tuple, list)) else (out,)):
        if torch.is_tensor(t):
            t.record_stream(main)
    return out, done


def nhwc_to_nchw_view(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)


def nchw_view_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    y = x.permute(0, 2, 3, 1)
    return y if y.is_contiguous() else y.contiguous()


def weight_krsc(w: torch.Tensor) -> torch.Tensor:
    """OIHW parameter (channels_last storage) -> (Cout,R,S,Cin) contiguous view (copy only if the
    parameter is not channels_last, e.g. a foreign checkpoint tensor assigned by hand).  A 5-D Conv3d weight
    (Cout, Cin, kt, kh, kw) in channels_last_3d storage gives (Cout, kt, 1, Cin) for a kt x 1 x 1 filter and
    (Cout, kh, kw, Cin) for a 1 x kh x kw filter (the two kinds an I3D bottleneck has)."""
    if w.dim() == 5:
        co, ci, kt, kh, kw = w.shape
        if kt > 1 and (kh > 1 or kw > 1):
            raise NotImplementedError('weight_krsc: a filter that is both temporal and spatial (only the I3D stem has one)')
        v = w.permute(0, 2, 3, 4, 1)
        v = v if v.is_contiguous() else v.contiguous()
        return v.reshape(co, kt, 1, ci) if kt > 1 else v.reshape(co, kh, kw, ci)
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def grad_like_weight(dw_krsc: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """(Cout,R,S,Cin) kernel output -> a gradient of the parameter's logical shape (a view: its storage is the parameter's)."""
    if w.dim() == 5:
        co, ci, kt, kh, kw = w.shape
        return dw_krsc.reshape(co, kt, kh, kw, ci).permute(0, 4, 1, 2, 3)
    return dw_krsc.permute(0, 3, 1, 2)


class UnitSpec:
    """Static description of one conv+BN(+ReLU) site inside a block."""

    def __init__(self, cin, cout, k, stride, pad, relu, shift_div=0, num_segments=1):
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, pad, relu
        self.fold = cin // shift_div if shift_div else 0
        self.T = num_segments if shift_div else 1

    def geom(self, N, H, W):
        return K.make_geom(N, H, W, self.cin, self.cout, self.k, self.k, self.stride, self.pad, self.T, self.fold)

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1


class TemporalUnitSpec(UnitSpec):
    """kt x 1 x 1 convolution + BN(+ReLU) of an I3D bottleneck: per frame nothing changes spatially; the conv runs on the
    [B][T][H*W][C] view of the frames (``frames`` per clip = T)."""

    def __init__(self, cin, cout, kt, relu, frames):
        super().__init__(cin, cout, 1, 1, 0, relu)
        self.kt, self.frames = kt, frames

    def geom(self, N, H, W):
        if N % self.frames:
            raise ValueError(f'{N} frames are not whole clips of {self.frames}')
        return K.make_temporal_geom(N // self.frames, self.frames, H, W, self.cin, self.cout, self.kt)

    def out_hw(self, H, W):
        return H, W


def _conv_bn_forward(x, w_krsc, g, bn, gamma, beta, training, pre_bn=None):
    """conv + BatchNorm statistics -> (y, mean, invstd, scale, shift) in training mode: the batch statistics come out
    of the conv epilogue (no extra pass over y) and running stats are updated in place.  ``pre_bn``: (scale, shift) of the
    producing unit when x is its raw conv output (its BatchNorm + ReLU is applied in this conv's loader)."""
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm momentum=None (cumulative average) is not supported by the HIP path')
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    y, part = K.conv_fprop(x, w_krsc, g, bn_stats=True, pre_bn=pre_bn)
    mean, invstd, scale, shift = K.bn_train_finalize(part, g.N * g.Ho * g.Wo, gamma, beta, bn.eps, bn.momentum, rm, rv)
    return y, mean, invstd, scale, shift


def _conv_bn_eval(x, w_krsc, g, bn, gamma, beta, res, relu):
    """Eval-mode conv + BatchNorm (+ residual) (+ ReLU) in one kernel: the running statistics fold into a per-channel
    scale / shift applied in the conv epilogue."""
    scale, shift = K.bn_eval_params(gamma, beta, bn.running_mean, bn.running_var, bn.eps)
    return K.conv_fprop(x, w_krsc, g, affine=(scale, shift, res, relu))


def _bn_wgrad_backward(dout, mask, y, gamma, mean, invstd, inp, geom, need_dw, stat_partial=None, relu_affine=None, pre_bn=None):
    """BatchNorm(+ReLU) backward of one conv+BN unit followed by the conv's wgrad -> (dy, dgamma, dbeta, dw | None).
    ``relu_affine``: (scale, shift) of THIS unit when its mask was never written (the sign is derived from y);
    ``pre_bn``: (scale, shift) of the unit that produced ``inp`` when ``inp`` is that unit's raw conv output."""
    dy, dg, db = K.bn_backward(dout, mask, y, gamma, mean, invstd, True, stat_partial=stat_partial, relu_affine=relu_affine)
    dw = wgrad_overlapped(dy, inp, geom, pre_bn=pre_bn) if need_dw else None
    return dy, dg, db, dw


def save_plan(needs_input_grad, training, grad):
    """-> (save, eval_grad) of a node's forward.  ``eval_grad``: it runs the differentiable eval-mode-BatchNorm form -- something
    behind it needs a gradient, its BatchNorms are in eval mode and the caller records a graph (``grad`` = torch.is_grad_enabled()
    at the call: inside Function.forward it is always off).  ``save``: it keeps tensors for a backward pass.  Inference keeps the
    fused eval kernels and saves nothing; so does bf16 activation storage, whose backward then raises."""
    need = any(needs_input_grad)
    eval_grad = bool(need and not training and grad and K.ACT_DTYPE == torch.float32)
    return bool(need and (training or eval_grad)), eval_grad


def require_eval_backward(ctx):
    """First statement of a node's backward: a node that ran its eval-mode forward without the differentiable form (bf16 activation
    storage) has nothing saved."""
    if not ctx.bn_training and not ctx.eval_grad:
        _require_fp32_storage()
        raise NotImplementedError('backward through an eval-mode BatchNorm forward that ran with gradient recording off')


def _require_fp32_storage():
    if K.ACT_DTYPE != torch.float32:
        raise NotImplementedError("backward through eval-mode BatchNorm (norm_eval / frozen_stages / partial_bn, or a BatchNorm in "
                                  ".eval() inside a training step) is not implemented for bf16 activation storage "
                                  "(set_conv_arith('bf16')); the other arithmetics keep fp32 tensors and are supported")


def _sign_bits(a):
    """1-bit sign mask (a > 0) of an activation tensor, for RELU_MASK_TAP only: the units whose BatchNorm affine is frozen write
    no mask of their own (their backward reads the sign off the activation)."""
    one, zero = K.bn_unit_affine(a.shape[-1], a.device)
    return K.bn_apply(a, one, zero, None, True, want_mask=True)[1]


class StemFn(torch.autograd.Function):
    """UPSTREAM ResNet.conv1 (7x7/2 ConvModule) + ResNet.maxpool on NHWC4 input."""

    @staticmethod
    def forward(ctx, x4, weight, gamma, beta, bn, training, grad=True):
        N, H, W, _ = x4.shape
        g = K.make_geom(N, H, W, 4, weight.shape[0], weight.shape[2], weight.shape[3], 2, weight.shape[2] // 2)
        w4 = torch.zeros((weight.shape[0], weight.shape[2], weight.shape[3], 4), dtype=torch.float32, device=x4.device)
        w4[..., :3] = weight.detach().permute(0, 2, 3, 1)           # 37 KB repack, plumbing
        save, eval_grad = save_plan(ctx.needs_input_grad, training, grad)
        # eval-mode BatchNorm inside a training step: 'affine' = gamma / beta trainable (norm_eval), 'frozen' = statistics and affine
        # fixed (only the filter trains); None = train mode, or nothing behind this node needs a gradient
        mode = None
        if eval_grad:
            mode = 'affine' if (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]) else 'frozen'
        a_shape = (N, g.Ho, g.Wo, weight.shape[0])
        if training:
            y, mean, invstd, scale, shift = _conv_bn_forward(x4, w4, g, bn, gamma, beta, training)
            # BN apply + ReLU + max-pool + ReLU sign mask in one pass; the activation itself is never materialised
            p, idx, mask = K.bn_relu_maxpool_fwd(y, scale, shift, out_dtype=K.ACT_DTYPE)
            _tap_mask(y.shape, mask)
            _tap_pool(idx)
            if save:
                ctx.save_for_backward(x4, gamma, y, mask, idx, mean, invstd)
        elif mode == 'affine':
            # the conv without the statistics epilogue, then the train-mode tail on the running statistics' scale / shift
            y = K.conv_fprop(x4, w4, g)
            scale, shift = K.bn_eval_params(gamma, beta, bn.running_mean, bn.running_var, bn.eps)
            p, idx, mask = K.bn_relu_maxpool_fwd(y, scale, shift, out_dtype=K.ACT_DTYPE)
            _tap_mask(y.shape, mask)
            _tap_pool(idx)
            ctx.save_for_backward(x4, scale, y, mask, idx, bn.running_mean, K.bn_eval_invstd(bn.running_var, bn.eps))
        else:
            scale, shift = K.bn_eval_params(gamma, beta, bn.running_mean, bn.running_var, bn.eps)
            a = K.conv_fprop(x4, w4, g, affine=(scale, shift, None, True))
            p, idx = K.maxpool_fwd(a, out_dtype=K.ACT_DTYPE)
            if mode == 'frozen':
                _tap_mask(a.shape, lambda: _sign_bits(a))
                _tap_pool(idx)
                ctx.save_for_backward(x4, scale, a, idx)
        ctx.g = g
        ctx.bn_training = training
        ctx.eval_mode = mode
        ctx.eval_grad = eval_grad
        ctx.a_shape = a_shape
        return p

    @staticmethod
    def backward(ctx, dp):
        require_eval_backward(ctx)
        dp = dp if dp.is_contiguous() else dp.contiguous()
        dgamma = dbeta = None
        if ctx.bn_training:
            x4, gamma, y, mask, idx, mean, invstd = ctx.saved_tensors
            # max-pool backward + BN/ReLU backward in one go: the 822 MB gradient of the stem activation is never written
            dy, dgamma, dbeta = K.bn_backward_maxpool(dp, idx, mask, y, gamma, mean, invstd)
        elif ctx.eval_mode == 'affine':
            x4, scale, y, mask, idx, mean, invstd = ctx.saved_tensors
            da = K.maxpool_bwd(dp, idx, ctx.a_shape)
            dy, _, dgamma, dbeta = K.bn_eval_backward(da, scale, relu_mask=mask, y=y, running_mean=mean, invstd=invstd, want_params=True)
        else:
            x4, scale, a, idx = ctx.saved_tensors
            dy = K.bn_eval_backward(K.maxpool_bwd(dp, idx, ctx.a_shape), scale, relu_act=a)[0]
        dw = None
        if ctx.needs_input_grad[1]:
            dw4 = K.conv_wgrad(dy, x4, ctx.g)
            dw = dw4[..., :3].permute(0, 3, 1, 2)
        join_side_stream(dp.device)          # the stem is the last backward node: all wgrads are visible after it
        return None, dw, dgamma, dbeta, None, None, None


class UnitParams(NamedTuple):
    """(weight, gamma, beta) of one conv+BN unit; also: which of the three need a gradient, and their gradients."""
    weight: object
    gamma: object
    beta: object


def split_params(params) -> List[UnitParams]:
    """Flat (weight, gamma, beta, weight, ...) as an autograd node receives it -> one record per unit."""
    return [UnitParams(*params[k:k + 3]) for k in range(0, len(params), 3)]


def split_need(needs, offset) -> List[UnitParams]:
    """``needs_input_grad`` of a node whose parameters start at position ``offset`` of ``apply(...)`` -> one record per unit."""
    return split_params(needs[offset:])


def _flat(records) -> list:
    return [t for r in records for t in r]


class UnitSaved(NamedTuple):
    """What the forward of one conv+BN(+ReLU) unit keeps for its backward: ``y`` the raw conv output, ``act`` the activation after
    BatchNorm (+ residual) + ReLU, ``mask`` its 1-bit ReLU signs.  Fields set (others None), by the form the unit ran in:

        train mode                      y  act  mean          invstd          mask
        train mode, apply deferred      y       mean          invstd                scale  shift
        eval mode, affine live          y  act  running_mean  of running_var  mask  scale
        eval mode, affine frozen           act                                      scale
        downsample, train mode          y       mean          invstd
        downsample, eval mode, live     y       running_mean  of running_var        scale
        downsample, eval mode, frozen                                               scale

    Apply deferred (``PRE_BN``): the consumer conv applies this unit's BatchNorm + ReLU in its loaders; the backward kernels derive
    the sign from ``y`` and (scale, shift).  Eval mode: BatchNorms on their running statistics inside a training step (UPSTREAM
    norm_eval / partial_bn / frozen_stages, a user's .eval()), per unit by whether its gamma / beta need a gradient.  Live: conv ->
    bn_apply with the eval scale / shift; backward = bn_eval_backward with dgamma / dbeta.  Frozen: the fused eval kernel (conv +
    folded BatchNorm + residual + ReLU); only the activation is kept -- the operand of the next weight gradient anyway -- and the
    backward reads the ReLU sign off it.  The downsample branch shares the block output's mask."""
    y: Optional[torch.Tensor] = None
    act: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    invstd: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    # train mode: (scale, shift) of a unit whose apply pass was deferred, else None
    pre_bn = property(lambda self: (self.scale, self.shift) if self.scale is not None else None)

    def bn_stat_operands(self):
        """(y, mask, mean, invstd), the order ``K.conv_dgrad(bn_stats=...)`` documents: what a dgrad epilogue needs to take the
        BatchNorm-backward statistics of the gradient it writes into this unit's output."""
        return self.y, self.mask, self.mean, self.invstd


class BlockSaved(NamedTuple):
    """Saved tensors of one block: its input, one ``UnitSaved`` per main unit, one for a downsample branch; flat for autograd."""
    x: torch.Tensor
    units: Sequence[UnitSaved]
    down: Optional[UnitSaved]

    def flatten(self) -> list:
        return [self.x] + _flat(self.units) + list(self.down or ())

    @classmethod
    def unflatten(cls, tensors, n_main, has_down):
        q = len(UnitSaved._fields)
        units = [UnitSaved(*tensors[1 + q * i:1 + q * (i + 1)]) for i in range(n_main + has_down)]
        return cls(tensors[0], units[:n_main], units[n_main] if has_down else None)


class BlockPlan(NamedTuple):
    """What an autograd node remembers about one block besides tensors.  ``geoms``: one per unit, the downsample's last."""
    geoms: list
    n_main: int
    has_down: bool
    n_units = property(lambda self: self.n_main + self.has_down)
    n_params = property(lambda self: len(UnitParams._fields) * self.n_units)
    n_saved = property(lambda self: 1 + len(UnitSaved._fields) * self.n_units)      # = len(BlockSaved.flatten())


def split_stage(plans, tensors, needs, offset):
    """``tensors``: what a node over the blocks ``plans`` saved (every block's ``flatten()``, then every block's parameters);
    ``needs``: its needs_input_grad.  -> per block (BlockSaved, [UnitParams], [UnitParams of needs])."""
    units, need = split_params(tensors[sum(p.n_saved for p in plans):]), split_need(needs, offset)
    out, s, u = [], 0, 0
    for p in plans:
        saved = BlockSaved.unflatten(tensors[s:s + p.n_saved], p.n_main, p.has_down)
        out.append((saved, units[u:u + p.n_units], need[u:u + p.n_units]))
        s, u = s + p.n_saved, u + p.n_units
    return out


def _block_forward(x, blk, training, params, save, need=None, eval_grad=False):
    """Forward of one residual block (UPSTREAM BasicBlock / Bottleneck, shift_place='blockres') on NHWC storage.
    ``params``: one UnitParams per unit; ``need``: which of them need a gradient (read by the eval-mode form that is
    differentiated).  Returns (out, BlockSaved for backward | None, BlockPlan)."""
    if eval_grad:
        return _block_forward_eval_grad(x, blk, params, need)
    units, bns, n_main = blk.unit_specs, blk.unit_bns, blk.n_main
    has_down = len(units) > n_main
    N, H, W, _ = x.shape
    saved, geoms, down, ds_event = [], [], None, None
    # identity path
    if has_down:
        (wd, gd, bd), g = params[n_main], units[n_main].geom(N, H, W)
        if training:
            # the downsample BatchNorm is applied inside the block-output kernel (res_affine): no identity tensor
            if DS_SIDE and _SIDE['enabled'] and x.is_cuda:
                (yd, mean_d, invstd_d, sc_d, sh_d), ds_event = run_on_side_stream(
                    lambda: _conv_bn_forward(x, weight_krsc(wd), g, bns[n_main], gd, bd, training), x.device)
                x.record_stream(_side_stream(x.device)[1])
            else:
                yd, mean_d, invstd_d, sc_d, sh_d = _conv_bn_forward(x, weight_krsc(wd), g, bns[n_main], gd, bd, training)
            identity, id_affine = yd, (sc_d, sh_d)
            down = UnitSaved(y=yd, mean=mean_d, invstd=invstd_d)
        else:
            identity, id_affine = _conv_bn_eval(x, weight_krsc(wd), g, bns[n_main], gd, bd, None, False), None
    else:
        identity, id_affine = x, None
    cur, h, w_ = x, H, W
    pending = None          # (scale, shift) of the previous unit when `cur` is its raw conv output
    for i in range(n_main):
        u, (wt, gm, bt) = units[i], params[i]
        g = u.geom(N, h, w_)
        geoms.append(g)
        last = i == n_main - 1
        if not training:     # eval: conv + folded BatchNorm (+ identity) + ReLU in one kernel
            h, w_ = u.out_hw(h, w_)
            cur = _conv_bn_eval(cur, weight_krsc(wt), g, bns[i], gm, bt, identity if last else None, True).view(N, h, w_, u.cout)
            continue
        y, mean, invstd, sc, sh = _conv_bn_forward(cur, weight_krsc(wt), g, bns[i], gm, bt, training, pre_bn=pending)
        y = y.view(N, *u.out_hw(h, w_), u.cout)          # frames view (a temporal geometry describes another view of it)
        if last and has_down and training and ds_event is not None:
            torch.cuda.current_stream(x.device).wait_event(ds_event)      # the identity branch is needed from here on
        h2, w2 = u.out_hw(h, w_)
        # the next unit of the main branch can apply this unit's BatchNorm + ReLU in its own loaders: no apply pass here
        if not last and PRE_BN and K.fprop_pre_ok(units[i + 1].geom(N, h2, w2)):
            # tests read every ReLU's sign bits: produce them on the side
            _tap_mask(y.shape, lambda: K.bn_apply(y, sc, sh, None, True, want_mask=True)[1])
            if save:
                saved.append(UnitSaved(y=y, mean=mean, invstd=invstd, scale=sc, shift=sh))
            cur, pending = y, (sc, sh)
        else:
            if save:
                a, mask = K.bn_apply(y, sc, sh, identity if last else None, True, want_mask=True,
                                     res_affine=id_affine if last else None)
                saved.append(UnitSaved(y, a, mean, invstd, mask))
                _tap_mask(y.shape, mask)
            else:
                a = K.bn_apply(y, sc, sh, identity if last else None, True, res_affine=id_affine if last else None)
            cur, pending = a, None
        h, w_ = h2, w2
    if save and has_down:
        geoms.append(units[n_main].geom(N, H, W))
    return cur, (BlockSaved(x, saved, down) if save else None), BlockPlan(geoms, n_main, has_down)


def _block_backward(saved, params, plan, dout, need, need_dx, out_stat_partial=None, prev_stats=None):
    """Backward of one residual block.  ``out_stat_partial``: tile sums of the BatchNorm-backward statistics of ``dout``
    against this block's last unit, when the producer of ``dout`` already took them.  ``prev_stats``: statistics
    operands of the PREVIOUS block's last unit; the dgrad that writes dx then reduces them in its epilogue.
    Returns (dx, parameter gradients in the order of the node's ``*params``, partial for the previous block | None)."""
    x, units, down = saved
    geoms, n_main, k = plan.geoms, plan.n_main, plan.n_main - 1
    out_mask = units[k].mask
    dout = dout if dout.is_contiguous() else dout.contiguous()
    grads = [UnitParams(None, None, None)] * len(params)
    # main branch, last unit first.  ``d`` is the gradient w.r.t. the unit's (post-ReLU) output.
    d, part = dout, out_stat_partial
    # A downsample branch: the masked gradient dout * (out > 0) enters two BatchNorms, the last main unit's and the downsample's.
    # One pair call reads dout and the mask once per pass for both (plain mask form only: a unit whose sign is derived from y
    # keeps the two-call path).
    pair_down = None
    if plan.has_down and units[k].pre_bn is None and out_mask is not None:
        pair_main, pair_down = K.bn_backward_pair(dout, out_mask, units[k].y, params[k].gamma, units[k].mean, units[k].invstd, down.y,
                                                  params[n_main].gamma, down.mean, down.invstd, stat_partial_a=part)
    for i in range(k, -1, -1):
        u, p, prev = units[i], params[i], units[i - 1] if i > 0 else None
        # this conv's input: the previous unit's activation, or its raw conv output + (scale, shift) for the loader
        inp = x if prev is None else (prev.act if prev.pre_bn is None else prev.y)
        pre_bn = prev.pre_bn if prev is not None else None
        if i == k and pair_down is not None:
            dy, dg, db = pair_main
            dw = wgrad_overlapped(dy, inp, geoms[i], pre_bn=pre_bn) if need[i].weight else None
        else:
            dy, dg, db, dw = _bn_wgrad_backward(d, u.mask, u.y, p.gamma, u.mean, u.invstd, inp, geoms[i], need[i].weight,
                                                stat_partial=part, relu_affine=u.pre_bn, pre_bn=pre_bn)
        grads[i] = UnitParams(grad_like_weight(dw, p.weight) if dw is not None else None, dg, db)
        part = None
        if i > 0:
            gi = geoms[i]
            if FUSE_BN_STATS and (gi.stride == 1 or (gi.R > 1 and gi.S > 1 and gi.fold == 0)):
                # this dgrad produces the gradient entering unit i-1's BN+ReLU: take its statistics in the epilogue
                # (stride 2: a 3x3 filter reaches every input pixel, one block of partial rows per parity class)
                stats = prev.bn_stat_operands()
                d, part = K.conv_dgrad(dy, weight_krsc(p.weight), gi, bn_stats=stats if pre_bn is None else stats + (pre_bn,))
            else:
                d = K.conv_dgrad(dy, weight_krsc(p.weight), gi)
            d = d.view_as(inp)                     # frames view (the geometry of a temporal conv names another view)
        else:
            dy_first = dy
    dx, prev_partial = None, None
    stats = prev_stats if (FUSE_BN_STATS and prev_stats is not None and geoms[0].stride == 1) else None
    if plan.has_down:
        (wd, gd, _), gdn, need_dwd = params[n_main], geoms[n_main], need[n_main].weight
        # gradient entering the downsample BN is dout * (out > 0): same mask as the block output
        if pair_down is not None:
            dyd, dgd, dbd = pair_down
            dwd = wgrad_overlapped(dyd, x, gdn) if need_dwd else None
        else:
            dyd, dgd, dbd, dwd = _bn_wgrad_backward(dout, out_mask, down.y, gd, down.mean, down.invstd, x, gdn, need_dwd)
        grads[n_main] = UnitParams(grad_like_weight(dwd, wd) if dwd is not None else None, dgd, dbd)
        if need_dx:
            dx_id = K.conv_dgrad(dyd, weight_krsc(wd), gdn)
            dx = K.conv_dgrad(dy_first, weight_krsc(params[0].weight), geoms[0], add_src=dx_id, bn_stats=stats)
    elif need_dx:
        # identity path: dout * (out > 0), fused into the conv1 dgrad epilogue
        dx = K.conv_dgrad(dy_first, weight_krsc(params[0].weight), geoms[0], add_src=dout, add_mask_src=out_mask, bn_stats=stats)
    if stats is not None and dx is not None:
        dx, prev_partial = dx
    if dx is not None:
        dx = dx.view_as(x)
    return dx, _flat(grads), prev_partial


def _block_forward_eval_grad(x, blk, params, need):
    """Forward of a block whose BatchNorms run on their running statistics inside a training step, in the form that is
    differentiated: per unit the live or the frozen form of the ``UnitSaved`` table, by whether its gamma / beta need a gradient."""
    units, bns, n_main = blk.unit_specs, blk.unit_bns, blk.n_main
    has_down = len(units) > n_main
    N, H, W, _ = x.shape

    def live(i):
        return bool(need[i].gamma or need[i].beta)

    def eval_affine(i):
        return K.bn_eval_params(params[i].gamma, params[i].beta, bns[i].running_mean, bns[i].running_var, bns[i].eps)

    saved, geoms = [], []
    identity, id_affine, down = x, None, None
    if has_down:
        wd, gdn = params[n_main].weight, units[n_main].geom(N, H, W)
        sc_d, sh_d = eval_affine(n_main)
        if live(n_main):
            yd = K.conv_fprop(x, weight_krsc(wd), gdn)
            if live(n_main - 1):        # the block-output pass applies the downsample BatchNorm itself (res_affine)
                identity, id_affine = yd, (sc_d, sh_d)
            else:                       # the fused kernel of a frozen last unit takes a finished residual
                identity = K.bn_apply(yd, sc_d, sh_d, None, False)
            down = UnitSaved(y=yd, mean=bns[n_main].running_mean, invstd=K.bn_eval_invstd(bns[n_main].running_var, bns[n_main].eps),
                             scale=sc_d)
        else:
            identity = K.conv_fprop(x, weight_krsc(wd), gdn, affine=(sc_d, sh_d, None, False))
            down = UnitSaved(scale=sc_d)
    cur, h, w_ = x, H, W
    for i in range(n_main):
        u = units[i]
        g = u.geom(N, h, w_)
        geoms.append(g)
        last = i == n_main - 1
        h2, w2 = u.out_hw(h, w_)
        w, (sc, sh) = weight_krsc(params[i].weight), eval_affine(i)
        if live(i):
            y = K.conv_fprop(cur, w, g).view(N, h2, w2, u.cout)
            a, mask = K.bn_apply(y, sc, sh, identity if last else None, True, want_mask=True, res_affine=id_affine if last else None)
            saved.append(UnitSaved(y, a, bns[i].running_mean, K.bn_eval_invstd(bns[i].running_var, bns[i].eps), mask, sc))
            _tap_mask(a.shape, mask)
        else:
            a = K.conv_fprop(cur, w, g, affine=(sc, sh, identity if last else None, True)).view(N, h2, w2, u.cout)
            saved.append(UnitSaved(act=a, scale=sc))
            _tap_mask(a.shape, lambda: _sign_bits(a))
        cur, h, w_ = a, h2, w2
    if has_down:
        geoms.append(gdn)
    return cur, BlockSaved(x, saved, down), BlockPlan(geoms, n_main, has_down)


def _block_backward_eval(saved, params, plan, dout, need, need_dx):
    """Backward of ``_block_forward_eval_grad``: one bn_eval_backward pass per unit (no statistics hand-over between kernels:
    dy does not depend on the sums).  Returns (dx, parameter gradients, None)."""
    x, units, down = saved
    geoms, n_main, k = plan.geoms, plan.n_main, plan.n_main - 1
    out_mask = units[k].mask
    dout = dout if dout.is_contiguous() else dout.contiguous()
    grads = [UnitParams(None, None, None)] * len(params)
    d, dz_out, dy_first = dout, None, None
    for i in range(k, -1, -1):
        u, wt = units[i], params[i].weight
        inp = units[i - 1].act if i > 0 else x
        # the masked gradient of the block output also enters the downsample BatchNorm, or -- without one -- the identity path,
        # which re-derives it from (dout, mask) in the conv1 dgrad epilogue where a mask exists
        want_dz = i == k and (plan.has_down or (need_dx and out_mask is None))
        if u.y is not None:            # affine live
            dy, dz, dg, db = K.bn_eval_backward(d, u.scale, relu_mask=u.mask, y=u.y, running_mean=u.mean, invstd=u.invstd,
                                                want_params=True, want_dz=want_dz)
        else:                          # affine frozen: the sign off the activation, no parameter gradients (dg = db = None)
            dy, dz, dg, db = K.bn_eval_backward(d, u.scale, relu_act=u.act, want_dz=want_dz)
        if i == k:
            dz_out = dz
        dw = grad_like_weight(wgrad_overlapped(dy, inp, geoms[i]), wt) if need[i].weight else None
        grads[i] = UnitParams(dw, dg, db)
        if i == 0:
            dy_first = dy
        elif need_dx or any(any(n) for n in need[:i]):
            d = K.conv_dgrad(dy, weight_krsc(wt), geoms[i]).view_as(inp)
        else:
            break                      # nothing below this unit needs a gradient
    dx = None
    if plan.has_down:
        wd, gdn = params[n_main].weight, geoms[n_main]
        dgd = dbd = None
        if down.y is not None:
            dyd, _, dgd, dbd = K.bn_eval_backward(dz_out, down.scale, y=down.y, running_mean=down.mean, invstd=down.invstd,
                                                  want_params=True)
        elif need[n_main].weight or need_dx:
            dyd = K.bn_eval_backward(dz_out, down.scale)[0]
        dwd = grad_like_weight(wgrad_overlapped(dyd, x, gdn), wd) if need[n_main].weight else None
        grads[n_main] = UnitParams(dwd, dgd, dbd)
        if need_dx:
            dx_id = K.conv_dgrad(dyd, weight_krsc(wd), gdn)
            dx = K.conv_dgrad(dy_first, weight_krsc(params[0].weight), geoms[0], add_src=dx_id)
    elif need_dx:
        if out_mask is not None:
            dx = K.conv_dgrad(dy_first, weight_krsc(params[0].weight), geoms[0], add_src=dout, add_mask_src=out_mask)
        else:
            dx = K.conv_dgrad(dy_first, weight_krsc(params[0].weight), geoms[0], add_src=dz_out)
    if dx is not None:
        dx = dx.view_as(x)
    return dx, _flat(grads), None


class ResBlockFn(torch.autograd.Function):
    """One residual block as an autograd node (used when a stage cannot run as one node, e.g. hooks on its blocks)."""

    @staticmethod
    def forward(ctx, x, blk, training, grad, *params):
        save, eval_grad = save_plan(ctx.needs_input_grad, training, grad)
        first = len(ctx.needs_input_grad) - len(params)
        out, saved, ctx.plan = _block_forward(x, blk, training, split_params(params), save, split_need(ctx.needs_input_grad, first),
                                              eval_grad)
        if save:
            ctx.save_for_backward(*saved.flatten(), *params)
        ctx.bn_training = training
        ctx.eval_grad = eval_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        require_eval_backward(ctx)
        need = ctx.needs_input_grad
        first = len(need) - ctx.plan.n_params        # (x, blk, training, grad, *params)
        (saved, params, need_params), = split_stage([ctx.plan], ctx.saved_tensors, need, first)
        backward = _block_backward if ctx.bn_training else _block_backward_eval
        with wgrad_batch():
            dx, grads, _ = backward(saved, params, ctx.plan, dout, need_params, need[0])
        if not need[0]:
            join_side_stream(dout.device)    # nothing below needs a gradient (frozen stem / stages): the last backward node
        return (dx, *[None] * (first - 1), *grads)


class StageLink:
    """Side channel between two consecutive stages run as ResStageFn nodes, valid only while the first stage's output has the
    second stage as its ONLY consumer (no hook on the stage module): the producer leaves the BatchNorm-backward operands of its
    last unit (``stats``), the consumer's backward -- whose first conv1 dgrad writes the gradient w.r.t. that output -- takes their
    statistics in its epilogue and leaves the tile sums (``partial``) for the producer's backward, which runs after it."""
    __slots__ = ('stats', 'partial')

    def __init__(self):
        self.stats = None
        self.partial = None


CROSS_STAGE_STATS = _os.environ.get('BDVCIL_CROSS_STAGE_STATS', '1') != '0'


class ResStageFn(torch.autograd.Function):
    """A whole stage (UPSTREAM ResNet.layerN = a sequence of residual blocks) as ONE autograd node.  The tensors
    between its blocks are then private to this node (exactly one producer and one consumer), which is what allows
    block k+1's conv1 dgrad -- the kernel that writes the gradient w.r.t. block k's output -- to take the
    BatchNorm-backward statistics of block k's last unit in its epilogue instead of a separate pass over that
    (widest) tensor.  Arithmetic per block is that of ResBlockFn."""

    @staticmethod
    def forward(ctx, x, blocks, training, in_link, out_link, grad, *params):
        save, eval_grad = save_plan(ctx.needs_input_grad, training, grad)
        first = len(ctx.needs_input_grad) - len(params)
        units, need = split_params(params), split_need(ctx.needs_input_grad, first)
        cur, all_saved, plans = x, [], []
        for blk in blocks:
            u, n = sum(p.n_units for p in plans), len(blk.unit_bns)
            cur, saved, plan = _block_forward(cur, blk, training, units[u:u + n], save, need[u:u + n], eval_grad)
            all_saved.append(saved)
            plans.append(plan)
        # the previous stage's last unit: operands for the statistics this stage's first conv1 dgrad can take for it
        # (train mode only: an eval-mode BatchNorm's backward has no statistics to hand over)
        in_stats = in_link.stats if (save and training and in_link is not None and CROSS_STAGE_STATS and FUSE_BN_STATS) else None
        if in_stats is not None and not (plans[0].geoms[0].stride == 1 and ctx.needs_input_grad[0]):
            in_stats = None
        if save:
            ctx.save_for_backward(*[t for s in all_saved for t in s.flatten()], *params, *(in_stats or ()))
            if out_link is not None and training:
                out_link.stats = all_saved[-1].units[-1].bn_stat_operands()
        ctx.in_link = in_link if in_stats is not None else None
        ctx.out_link = out_link if (save and training) else None
        ctx.plans = plans
        ctx.bn_training = training
        ctx.eval_grad = eval_grad
        return cur

    @staticmethod
    def backward(ctx, dout):
        require_eval_backward(ctx)
        t, in_stats = ctx.saved_tensors, None
        if ctx.in_link is not None:
            t, in_stats = t[:-4], tuple(t[-4:])
        need = ctx.needs_input_grad
        first = len(need) - sum(p.n_params for p in ctx.plans)     # (x, blocks, training, in_link, out_link, grad, *params)
        blocks = split_stage(ctx.plans, t, need, first)
        grads_all = [[None] * p.n_params for p in ctx.plans]
        d, part = dout, None
        if ctx.out_link is not None:     # the next stage's backward ran before this one and took the statistics of `dout`
            part, ctx.out_link.partial = ctx.out_link.partial, None
        with wgrad_batch():              # one split-K reduction launch for the weight gradients of the whole stage
            for k in range(len(blocks) - 1, -1, -1):
                saved, params, need_params = blocks[k]
                if not ctx.bn_training:
                    # a block's dx feeds the blocks below it: not needed once nothing below needs a gradient
                    need_dx = need[0] or any(any(n) for _, _, below in blocks[:k] for n in below)
                    d, grads_all[k], part = _block_backward_eval(saved, params, ctx.plans[k], d, need_params, need_dx)
                    if d is None:
                        break
                    continue
                prev_stats = blocks[k - 1][0].units[-1].bn_stat_operands() if k > 0 else in_stats
                d, grads_all[k], part = _block_backward(saved, params, ctx.plans[k], d, need_params, need[0] or k > 0,
                                                        out_stat_partial=part, prev_stats=prev_stats)
        if ctx.in_link is not None:
            ctx.in_link.partial = part   # tile sums of the statistics of `d` against the previous stage's last unit
        if not need[0]:
            join_side_stream(dout.device)    # nothing below needs a gradient (frozen stem / stages): the last backward node
        return (d, *[None] * (first - 1), *_flat(grads_all))


class AvgPoolFn(torch.autograd.Function):
    """UPSTREAM TSMHead.avg_pool = AdaptiveAvgPool2d(1) on an NCHW view of NHWC storage."""

    @staticmethod
    def forward(ctx, x_nchw):
        x = nchw_view_to_nhwc(x_nchw)
        ctx.in_shape = tuple(x.shape)
        ctx.in_dtype = x.dtype          # bf16 storage ends here: the pooled features and everything after them are fp32
        return K.avgpool_fwd(x).view(x.shape[0], x.shape[3], 1, 1)

    @staticmethod
    def backward(ctx, dout):
        N, H, W, C = ctx.in_shape
        d = dout.reshape(N, C)
        d = d if d.is_contiguous() else d.contiguous()
        return nhwc_to_nchw_view(K.avgpool_bwd(d, ctx.in_shape, ctx.in_dtype))


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return K.dropout(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dout):
        return K.dropout(dout.contiguous(), ctx.p, ctx.seed), None, None


class LSCFn(torch.autograd.Function):
    """libs/models/cil_heads/cosine_linear.py:27-43."""

    @staticmethod
    def forward(ctx, x, weights, out_features, nb_proxies):
        x = x.contiguous()
        sim, xn, wn, cb = K.lsc_fwd(x, weights, out_features, nb_proxies)
        ctx.save_for_backward(x, weights, xn, wn, cb)
        ctx.kp = (out_features, nb_proxies)
        return sim

    @staticmethod
    def backward(ctx, dsim):
        x, w, xn, wn, cb = ctx.saved_tensors
        Kc, P = ctx.kp
        dx, dw = K.lsc_bwd(dsim.contiguous(), x, w, xn, wn, cb, Kc, P, need_dw=ctx.needs_input_grad[1])
        return dx, dw, None, None


class LinearFn(torch.autograd.Function):
    """libs/models/cil_heads/inc_net.py:36-37."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return K.linear_fwd(x, weight, bias)

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dx, dw, db = K.linear_bwd(dout.contiguous(), x, w, need_dx=ctx.needs_input_grad[0], need_dw=need_w,
                                  need_db=ctx.has_bias)
        return dx, dw, (db if ctx.has_bias else None)


class ConsensusFn(torch.autograd.Function):
    """UPSTREAM AvgConsensus(dim=1): (B,T,K) -> (B,1,K)."""

    @staticmethod
    def forward(ctx, x):
        B, T, Kc = x.shape
        ctx.T = T
        return K.consensus_fwd(x.reshape(B * T, Kc).contiguous(), B, T).view(B, 1, Kc)

    @staticmethod
    def backward(ctx, dout):
        B, _, Kc = dout.shape
        return K.consensus_bwd(dout.reshape(B, Kc).contiguous(), ctx.T).view(B, ctx.T, Kc)


def _scale_by(grad_out: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """Upstream scalar gradient times a small saved tensor ((B,K) or (1,)); host-free."""
    return t * grad_out


class LSCLossFn(torch.autograd.Function):
    """libs/losses/lsc_loss.py:36-56; forward kernel also produces dsim and deta."""

    @staticmethod
    def forward(ctx, sim, targets, eta, margin, hinge, class_weights=None):
        loss, dsim, deta = K.lsc_loss(sim.contiguous(), targets.contiguous(), eta, margin, hinge, class_weights)
        ctx.save_for_backward(dsim, deta)
        return loss

    @staticmethod
    def backward(ctx, g):
        dsim, deta = ctx.saved_tensors
        return _scale_by(g, dsim), None, (_scale_by(g, deta) if ctx.needs_input_grad[2] else None), None, None, None


class SoftCEFn(torch.autograd.Function):
    """libs/cil/icarl.py:123-125 (soft targets) or plain mean cross-entropy (integer labels)."""

    @staticmethod
    def forward(ctx, score, soft_targets, labels):
        loss, dscore = K.softce_loss(score.contiguous(), soft_targets, labels)
        ctx.save_for_backward(dscore)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dscore,) = ctx.saved_tensors
        return _scale_by(g, dscore), None, None


class KDMSEFn(torch.autograd.Function):
    """nn.MSELoss() between hooked feature maps (libs/cil/cil.py:519-541); ``prev`` gets no gradient."""

    @staticmethod
    def forward(ctx, cur, prev):
        ctx.save_for_backward(cur, prev)
        return K.kd_mse_fwd(cur, prev)

    @staticmethod
    def backward(ctx, g):
        cur, prev = ctx.saved_tensors
        return K.kd_mse_bwd(cur, prev, g.reshape(1).contiguous(), 1.0), None


def kd_mse(cur: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    return KDMSEFn.apply(cur, prev.detach())


class KDPodSpatialFn(torch.autograd.Function):
    """PODNet's POD-spatial loss between hooked feature maps, in place of the MSE of libs/cil/cil.py:519-541 (csrc/pod_kd.hip).
    Saves ``cur`` and the profile gradient ``G`` only: the teacher's maps are free after the forward.  ``prev`` gets no gradient."""

    @staticmethod
    def forward(ctx, cur, prev):
        loss, G, cur_nhwc = K.pod_spatial_fwd(cur, prev)
        keep = cur_nhwc.permute(0, 3, 1, 2)          # cur itself when it is channels-last, else the one converted copy
        ctx.save_for_backward(cur if keep.stride() == cur.stride() else keep, G)
        ctx.cur_strides = cur.stride()
        return loss

    @staticmethod
    def backward(ctx, g):
        cur, G = ctx.saved_tensors
        d = K.pod_spatial_bwd(cur, G, g.reshape(1).to(torch.float32).contiguous())
        # pod_spatial_bwd answers in the strides of what it is given: the input itself when that was channels-last, otherwise the
        # converted copy saved above -- and then the gradient still has to take the input's own strides
        if d.stride() != ctx.cur_strides:
            d = torch.empty_strided(d.shape, ctx.cur_strides, dtype=d.dtype, device=d.device).copy_(d)
        return d, None


class KDPodFlatFn(torch.autograd.Function):
    """PODNet's POD-flat loss (F.cosine_embedding_loss, target 1) between pooled features, in place of the MSE of
    libs/cil/cil.py:519-541; the forward kernel also produces the gradient for an upstream gradient of 1."""

    @staticmethod
    def forward(ctx, cur, prev):
        loss, dunit = K.pod_flat(cur, prev)
        ctx.save_for_backward(dunit)
        ctx.cur_shape, ctx.cur_dtype = cur.shape, cur.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (dunit,) = ctx.saved_tensors
        return _scale_by(g, dunit).to(ctx.cur_dtype).view(ctx.cur_shape), None


def kd_pod_spatial(cur: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    return KDPodSpatialFn.apply(cur, prev.detach())


def kd_pod_flat(cur: torch.Tensor, prev: torch.Tensor) -> torch.Tensor:
    return KDPodFlatFn.apply(cur, prev.detach())


class KDTimeChannelFn(torch.autograd.Function):
    """The MSE of libs/cil/cil.py:519-541 weighted by a time-channel importance map (T, C): mean of
    ``importance[n mod T, c] * (cur - prev)^2`` over hooked outputs whose rows are frames n = b * T + t (csrc/tc_kd.hip).  Saves ``cur``,
    ``prev`` and the map; ``prev`` and the map get no gradient."""

    @staticmethod
    def forward(ctx, cur, prev, importance):
        ctx.save_for_backward(cur, prev, importance)
        return K.kd_tc_fwd(cur, prev, importance)

    @staticmethod
    def backward(ctx, g):
        cur, prev, importance = ctx.saved_tensors
        return K.kd_tc_bwd(cur, prev, importance, g.reshape(1).to(torch.float32).contiguous()), None, None


def kd_time_channel(cur: torch.Tensor, prev: torch.Tensor, importance: torch.Tensor) -> torch.Tensor:
    return KDTimeChannelFn.apply(cur, prev.detach(), importance.detach())
