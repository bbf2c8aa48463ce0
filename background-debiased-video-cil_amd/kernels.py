"""Tensor-level wrappers over the C ABI: shape/dtype/device checks on the host, then a launch on
torch's current HIP stream.  PyTorch is only the owner of device memory and streams here.

Every wrapper validates that operand shapes match what the kernel grid assumes BEFORE launching
(an out-of-bounds access on the GPU can reset the whole node).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from ._lib import BnStatFuse, ConvAffine, ConvGeom, ConvPlan, check, lib

_WS = {}  # (device index, tag) -> workspace tensor (grown on demand, never shrunk)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _chk(t: torch.Tensor, shape: Optional[Sequence[int]] = None, dtype=torch.float32, name='tensor'):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a tensor, got {type(t)}')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: the HIP path needs a GPU tensor (got device {t.device}); there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: dtype {t.dtype}, expected {dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: must be contiguous, got strides {t.stride()} for shape {tuple(t.shape)}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t


ACT_DTYPE = torch.float32       # storage type of activations / their gradients: torch.float32, or torch.bfloat16 ('bf16' arithmetic)


def _act_code(t: torch.Tensor) -> int:
    """BDV_ACT_F32 (0) | BDV_ACT_BF16 (1) of an activation tensor."""
    return 1 if t.dtype == torch.bfloat16 else 0


def _chk_act(t: torch.Tensor, shape=None, name='tensor', like: Optional[torch.Tensor] = None):
    """An activation operand: fp32, or bf16 in the bf16-storage mode; ``like``: must have that tensor's dtype."""
    if isinstance(t, torch.Tensor) and t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'{name}: dtype {t.dtype}, expected torch.float32 or torch.bfloat16')
    if like is not None and isinstance(t, torch.Tensor) and t.dtype != like.dtype:
        raise TypeError(f'{name}: dtype {t.dtype} differs from the other activation operand ({like.dtype})')
    return _chk(t, shape, dtype=t.dtype if isinstance(t, torch.Tensor) else torch.float32, name=name)


def _chk_conv(t: torch.Tensor, shape, g, name):
    """Operand check of a convolution.  A geometry marked ``frames_view`` (a k x 1 temporal convolution described on the
    [B][T][H*W][C] view) takes the usual [B*T][H][W][C] tensors of the same storage: element count and channel count must
    agree, the kernel only sees the pointer."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
        if g.act_dtype != 1:
            raise TypeError(f'{name}: bf16 tensor in an fp32 convolution call (operands of one call share the storage type)')
    elif g.act_dtype != 0:
        raise TypeError(f'{name}: dtype {getattr(t, "dtype", None)} in a bf16-storage convolution call')
    if getattr(g, 'frames_view', False):
        _chk(t, None, dtype=t.dtype, name=name)
        n = 1
        for d in shape:
            n *= d
        if t.numel() != n or t.shape[-1] != shape[-1]:
            raise ValueError(f'{name}: shape {tuple(t.shape)} is not a view of {tuple(shape)}')
        return t
    return _chk(t, shape, dtype=torch.bfloat16 if g.act_dtype == 1 else torch.float32, name=name)


def workspace(nbytes: int, device, tag='ws') -> torch.Tensor:
    key = (torch.device(device).index or 0, tag)
    cur = _WS.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = cur
    return cur


def make_geom(N, H, W, Cin, Cout, R, S, stride, pad, T=1, fold=0, pad_w=None, rt=0, st_t=0) -> ConvGeom:
    """``pad`` pads rows and columns unless ``pad_w`` gives the column padding separately (k x 1 temporal convolutions).
    ``rt`` > 1: the I3D stem's temporal taps (Cin = 4): N = output frames, T = output frames per clip, temporal stride ``st_t``;
    the input then has N * st_t frames and the weight is (Cout, rt * R, S, 4)."""
    pw = pad if pad_w is None else pad_w
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pw - S) // stride + 1
    return ConvGeom(N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, T, fold, -1 if pad_w is None else pad_w, rt, st_t)


def _in_frames(g: ConvGeom) -> int:
    return g.N * g.st_t if g.Rt > 1 else g.N


def _taps_r(g: ConvGeom) -> int:
    return g.R * g.Rt if g.Rt > 1 else g.R


def make_temporal_geom(B, T, H, W, Cin, Cout, kt) -> ConvGeom:
    """k x 1 x 1 temporal convolution (stride 1, padding k // 2) of [B*T][H][W][C] frames, as a k x 1 convolution on the
    [B][T][H*W][C] view of the same storage (I3D Bottleneck3d.conv1 with inflate, configs/_base_/models/i3d_r50.py:13)."""
    g = make_geom(B, T, H * W, Cin, Cout, kt, 1, 1, kt // 2, pad_w=0)
    g.frames_view = True
    return g


# ---------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------

WS_TAG_SUFFIX = ''     # set while launching on another stream: two streams must not share a K-split workspace


def _conv_ws(g: ConvGeom, kind: int, device, tag: str) -> torch.Tensor:
    need = lib().bdv_conv_workspace_bytes(ctypes.byref(g), kind)
    if need == 0:
        check(-1, 'bdv_conv_workspace_bytes')
    return workspace(need, device, tag + WS_TAG_SUFFIX)


import os as _os

# Arithmetic of the 128-wide convolution tiles.  Default: every fp32 product is formed from three
# bf16 pieces per operand (six v_mfma_f32_32x32x16_bf16 products of relative weight >= 2^-16, fp32 accumulate; the dropped
# terms are below 2^-24 relative, the level of fp32 rounding).  BDVCIL_CONV_F32MFMA=1 selects the v_mfma_f32_32x32x2_f32
# kernels (an exact fp32 FMA chain) for all three directions; the per-direction switches override it.
_F32MFMA = _os.environ.get('BDVCIL_CONV_F32MFMA', '0') != '0'


def _x3_default(name):
    v = _os.environ.get(name)
    return (not _F32MFMA) if v is None else v != '0'


FPROP_X3 = _x3_default('BDVCIL_FPROP_X3')


PIECES = 3      # 3: fp32-level products from three bf16 pieces per operand; 2: two pieces, three products ('bf16x2', 16 significand
                # bits); 1: single bf16 product (reduced precision, 'bf16x1'); 4: two fp16 pieces, three products ('f16x2', fp32 level)
F16X2 = 4       # BDV_ARITH_F16X2


def set_conv_arith(mode: str):
    """'bf16x3' (default), 'f32mfma', 'bf16x2' (two bf16 pieces per operand, three MFMA products, 16 significand bits; the plane
    kernels only, the other sites keep three pieces), 'f16x2' (two fp16 pieces of the operand times a per-tensor power of two, three
    MFMA products, fp32-level result; the same sites as 'bf16x2', the others keep three bf16 pieces; each operand tensor's maximum
    is taken on the device once, ``act_amax``), or the reduced-precision modes of BASELINE config 5: 'bf16x1' (operands rounded to bf16, one
    MFMA product, fp32 accumulate, fp32 tensors) and 'bf16' (the same arithmetic with activations and their gradients STORED as
    bf16 between the stem's max-pool and the average pool; fp32 statistics, weights and weight gradients) for fprop, dgrad and
    wgrad at once; returns the previous (fprop, dgrad, wgrad) flags.
    Leaving 'bf16x1' needs another ``set_conv_arith`` call (the flags alone do not restore ``PIECES``)."""
    global FPROP_X3, DGRAD_X3, WGRAD_X3, PIECES, ACT_DTYPE
    if mode not in ('bf16x3', 'f32mfma', 'bf16x2', 'f16x2', 'bf16x1', 'bf16'):
        raise ValueError(f"set_conv_arith: unknown mode {mode!r} ('bf16x3' | 'f32mfma' | 'bf16x2' | 'f16x2' | 'bf16x1' | 'bf16')")
    prev = (FPROP_X3, DGRAD_X3, WGRAD_X3)
    FPROP_X3 = DGRAD_X3 = WGRAD_X3 = (mode != 'f32mfma')
    PIECES = 1 if mode in ('bf16x1', 'bf16') else 2 if mode == 'bf16x2' else F16X2 if mode == 'f16x2' else 3
    _AMAX.clear()
    # 'bf16': the bf16x1 arithmetic on bf16-STORED activations and gradients (BDV_ACT_BF16) from the stem's max-pool to the average
    # pool; the tensors the model creates from here on carry the type, every kernel follows the dtype of what it is given
    ACT_DTYPE = torch.bfloat16 if mode == 'bf16' else torch.float32
    return prev


CONV_ARITH_MODES = ('bf16x3', 'f32mfma', 'bf16x2', 'f16x2', 'bf16x1', 'bf16')


def check_conv_arith(mode: str) -> str:
    """``mode`` if it is one of ``CONV_ARITH_MODES``, else ``ValueError``; touches nothing."""
    if mode not in CONV_ARITH_MODES:
        raise ValueError(f"conv_arith: unknown mode {mode!r} ({' | '.join(repr(m) for m in CONV_ARITH_MODES)})")
    return mode


def get_conv_arith() -> str:
    """The name ``set_conv_arith`` would need to produce the arithmetic in force, or 'custom' when no name does (a per-direction
    override: the BDVCIL_*_X3 environment switches, or a direct write of the flags)."""
    flags = (bool(FPROP_X3), bool(DGRAD_X3), bool(WGRAD_X3))
    if ACT_DTYPE == torch.bfloat16:
        return 'bf16' if flags == (True, True, True) and PIECES == 1 else 'custom'
    if flags == (False, False, False):
        return 'f32mfma' if PIECES == 3 else 'custom'
    if flags != (True, True, True):
        return 'custom'
    return {3: 'bf16x3', 2: 'bf16x2', F16X2: 'f16x2', 1: 'bf16x1'}.get(PIECES, 'custom')


import contextlib as _contextlib


@_contextlib.contextmanager
def conv_arith(mode: str):
    """``with conv_arith(mode):`` -- ``set_conv_arith(mode)`` for the body, and on the way out (normally or through an exception)
    everything that call writes is put back: the three direction flags, ``PIECES`` and ``ACT_DTYPE``, whatever they were (a 'custom'
    state included), and the cached operand maxima of 'f16x2' are dropped again.  Blocks nest.  An unknown mode raises ``ValueError``
    before anything changes.  Process-wide like ``set_conv_arith``: not for two threads that want different arithmetics."""
    global FPROP_X3, DGRAD_X3, WGRAD_X3, PIECES, ACT_DTYPE
    check_conv_arith(mode)
    saved = (FPROP_X3, DGRAD_X3, WGRAD_X3, PIECES, ACT_DTYPE)
    set_conv_arith(mode)
    try:
        yield mode
    finally:
        FPROP_X3, DGRAD_X3, WGRAD_X3, PIECES, ACT_DTYPE = saved
        _AMAX.clear()


# ---- weights as bf16 planes (bdv_conv_split_weights), cached per weight tensor -----------------------------------------
# A conv weight is cut into its hi / mid / lo planes once per value: the entry of a weight is refreshed when torch's version
# counter of the tensor moved (any in-place torch op, load_state_dict, torch optimizers), when its storage moved, or when
# WEIGHT_EPOCH moved -- the fused SGD kernel writes through raw pointers, which torch cannot see, so FusedSGD.step() calls
# bump_weight_epoch().  Forward and backward of one step share the planes; a frozen teacher's planes live as long as it does.
import weakref as _weakref

WEIGHT_EPOCH = 0
_PLANES = {}        # id(base tensor) -> [weakref, (data_ptr, version, epoch, fp16 pieces?), uint8 buffer holding both layouts, view,
                    # geometry, checksum]
# A write that torch's version counter does not see -- ``p.data.mul_()``, ``p.data.copy_()``, ``dist.broadcast(p.data)``, any kernel
# given ``p.data_ptr()`` -- leaves the stamp unchanged and the cached planes STALE: the convolutions would then run on the old
# weights without any error.  Such writers must call ``bump_weight_epoch()`` ("Weights written behind torch's
# back"); the writers inside this package (FusedSGD.step, broadcast_parameters) do.  BDVCIL_CHECK_PLANES=1 is the debugging aid for
# plugin code: every ``weight_planes`` hit then compares a checksum of the weight's bits with the one taken when the planes were
# cut (one device reduction and one host synchronisation per convolution: slow, never for timing) and raises on a mismatch.
CHECK_PLANES = _os.environ.get('BDVCIL_CHECK_PLANES', '0') != '0'


def _weight_checksum(w: torch.Tensor) -> int:
    return int(w.contiguous().view(torch.int32).to(torch.int64).sum().item())


def bump_weight_epoch(params=None):
    """Tell the plane cache that weights were changed behind torch's back (raw-pointer kernels): the given parameters, or
    every cached weight when ``params`` is None (a frozen teacher's planes survive the student's optimizer steps)."""
    global WEIGHT_EPOCH
    if params is None:
        WEIGHT_EPOCH += 1
        return
    for p in params:
        ent = _PLANES.get(id(p))
        if ent is not None:
            ent[1] = None


_PLANES_PENDING = {}    # device index -> (event of the last refresh_weight_planes() on another stream, streams ordered behind it)


def _plane_stamp(w, base, f16=False):
    return (w.data_ptr(), base._version, WEIGHT_EPOCH, bool(f16))


def _split_weights(w, g, buf, nbytes, f16):
    """Cut ``w`` into the planes of both layouts: three bf16 pieces, or (``f16``) two fp16 pieces and the weight's amax word."""
    if f16:
        check(lib().bdv_conv_split_weights_f16x2(_p(w), ctypes.byref(g), _p(buf[:nbytes]), _p(buf[nbytes:]), _stream()),
              'bdv_conv_split_weights_f16x2')
    else:
        check(lib().bdv_conv_split_weights(_p(w), ctypes.byref(g), _p(buf[:nbytes]), _p(buf[nbytes:]), _stream()),
              'bdv_conv_split_weights')


def weight_planes(w: torch.Tensor, g: ConvGeom, f16: bool = False):
    """(planes_fprop, planes_dgrad) of the (Cout, R, S, Cin) weight view ``w``: uint8 views of one cached buffer.  ``f16``: the
    planes of the 'f16x2' arithmetic (a weight has one kind at a time: the kernels of a site all read the same kind)."""
    if _PLANES_PENDING:
        pend = _PLANES_PENDING.get(w.device.index)
        if pend is not None:                            # (event, stream ids that are ordered behind it already)
            cur = torch.cuda.current_stream(w.device)
            if cur.cuda_stream not in pend[1]:
                cur.wait_event(pend[0])
                pend[1].add(cur.cuda_stream)
    base = w._base if w._base is not None else w
    key = id(base)
    stamp = _plane_stamp(w, base, f16)
    ent = _PLANES.get(key)
    if ent is not None and ent[0]() is not base:
        ent = None                                      # the id was recycled by another tensor
    nbytes = lib().bdv_conv_weight_planes_bytes(ctypes.byref(g))
    if nbytes == 0:
        check(-1, 'bdv_conv_weight_planes_bytes')
    if ent is None or ent[1] != stamp or ent[2].numel() != 2 * nbytes:
        buf = ent[2] if ent is not None and ent[2].numel() == 2 * nbytes and ent[2].device == w.device else \
            torch.empty(2 * nbytes, dtype=torch.uint8, device=w.device)
        _split_weights(w, g, buf, nbytes, f16)
        ref = _weakref.ref(base, lambda _r, k=key: _PLANES.pop(k, None))
        # how to rebuild the view and the geometry without holding the parameter alive (refresh_weight_planes)
        ent = [ref, stamp, buf, (tuple(w.shape), tuple(w.stride()), w.storage_offset()), (g.R, g.S, g.Cin, g.Cout),
               _weight_checksum(w) if CHECK_PLANES else None]
        _PLANES[key] = ent
    elif CHECK_PLANES and ent[5] is not None and _weight_checksum(w) != ent[5]:
        raise RuntimeError(
            'stale weight planes: a convolution weight of shape %s was changed without torch noticing (a write through `.data`, a '
            'raw-pointer kernel, dist.broadcast(p.data), ...) after its bf16 planes were cut, so fprop / dgrad would run on the OLD '
            'weights.  Call bdvcil_amd.bump_weight_epoch() after such a write (INTEGRATION.md).' % (tuple(w.shape),))
    return ent[2][:nbytes], ent[2][nbytes:]


def refresh_weight_planes(stream: Optional[torch.cuda.Stream] = None) -> int:
    """Re-split every cached weight whose planes are stale (after an optimizer step) in one go, on ``stream`` (default: the
    current one).  On another stream the work overlaps what the current stream does next (front-end, stem); the first
    ``weight_planes`` call afterwards makes its stream wait for it.  Returns the number of weights re-split."""
    n = 0
    by_dev = {}
    for key, ent in list(_PLANES.items()):
        base = ent[0]()
        if base is None or not base.is_cuda:
            continue
        shape, stride, off = ent[3]
        w = base.as_strided(shape, stride, off) if (tuple(base.shape), tuple(base.stride())) != (shape, stride) else base
        f16 = bool(ent[1][3]) if ent[1] is not None else PIECES == F16X2      # (bump_weight_epoch(params) clears the stamp)
        if ent[1] == _plane_stamp(w, base, f16):
            continue
        by_dev.setdefault(base.device, []).append((ent, w, base))
    for device, todo in by_dev.items():
        cur = torch.cuda.current_stream(device)
        st = stream if stream is not None and stream.device == device else cur
        if st != cur:
            st.wait_stream(cur)
        with torch.cuda.stream(st):
            for ent, w, base in todo:
                R, S, Cin, Cout = ent[4]
                g = make_geom(1, R, S, Cin, Cout, R, S, 1, 0, 1, 0)
                buf = ent[2]
                nbytes = buf.numel() // 2
                f16 = bool(ent[1][3]) if ent[1] is not None else PIECES == F16X2
                _split_weights(w, g, buf, nbytes, f16)
                ent[1] = _plane_stamp(w, base, f16)
                if CHECK_PLANES:
                    ent[5] = _weight_checksum(w)
                n += 1
            if st != cur:
                ev = torch.cuda.Event()
                ev.record(st)
                _PLANES_PENDING[device.index] = (ev, {st.cuda_stream})
    return n


# ---- 'f16x2': the amax word of an operand tensor (bdv_f16x2_amax), cached per tensor ------------------------------------------
# One HBM pass per tensor and value: x's word serves fprop and wgrad, dy's dgrad and wgrad, a block input's conv1 and the downsample.
# Keyed by the tensor a tensor views (views share their base's version counter) and the range viewed; an entry is valid while the
# version did not move and dies with the tensor.  Kernels of this package that write INTO a tensor they are given (``out=``, ``dy=``)
# call ``amax_forget``; plugin code that does the same through raw pointers must too.  R50 training step: about 100 passes.
_AMAX = {}          # id(base tensor) -> [weakref, {(data_ptr, numel): [version, int32 word, event, stream handle]}]


def act_amax(t: torch.Tensor) -> torch.Tensor:
    """The device-resident amax word (int32[1]: the bits of max|t|) of an fp32 activation / gradient tensor, computed on the current
    stream the first time it is asked for; no host synchronisation."""
    base = t._base if t._base is not None else t
    key = id(base)
    ent = _AMAX.get(key)
    if ent is not None and ent[0]() is not base:
        ent = None
    if ent is None:
        ent = _AMAX[key] = [_weakref.ref(base, lambda _r, k=key: _AMAX.pop(k, None)), {}]
    cur = torch.cuda.current_stream(t.device)
    sub = (t.data_ptr(), t.numel())
    rec = ent[1].get(sub)
    if rec is not None and rec[0] == base._version:
        if rec[3] != cur.cuda_stream:       # taken on another stream (a weight gradient on the side stream): order behind it
            cur.wait_event(rec[2])
        return rec[1]
    word = torch.empty(1, dtype=torch.int32, device=t.device)
    check(lib().bdv_f16x2_amax(_p(t), t.numel(), _p(word), _stream()), 'bdv_f16x2_amax')
    ev = torch.cuda.Event()
    ev.record(cur)
    ent[1][sub] = [base._version, word, ev, cur.cuda_stream]
    return word


def amax_forget(t):
    """``t`` was written by a raw-pointer kernel: its cached amax word (if any) is stale."""
    if _AMAX and isinstance(t, torch.Tensor):
        _AMAX.pop(id(t._base if t._base is not None else t), None)


def _plan_f16(plan) -> bool:
    """The plan runs the two-fp16-piece kernels (else, in 'f16x2', the call keeps three bf16 pieces)."""
    return plan.kernel.endswith(b'F16Pieces>')


def wgrad_amax(dy: torch.Tensor, x: torch.Tensor, g: ConvGeom):
    """'f16x2' only: take the amax words a weight gradient of this geometry will read, on the CURRENT stream (a caller that launches
    the weight gradient on another stream calls this first, so that other readers of the words do not wait for that stream)."""
    if PIECES != F16X2 or not WGRAD_X3 or dy.dtype != torch.float32 or x.dtype != torch.float32:
        return
    g.act_dtype = 0
    if _plan_f16(conv_plan(g, 'wgrad')):
        act_amax(dy)
        act_amax(x)


_KINDS = {'fprop': 0, 'dgrad': 1, 'wgrad': 2}


def conv_plan(g: ConvGeom, kind: str, x3: Optional[bool] = None, pre: bool = False) -> ConvPlan:
    """The library's plan of ``conv_fprop`` / ``conv_dgrad`` / ``conv_wgrad(_partial)`` for this geometry in the current arithmetic
    (``x3``: instead of the direction's flag; ``g.act_dtype`` as the caller set it; ``pre``: with ``pre_bn``): ``kernel``,
    ``reads_planes``, ``stat_rows``, ``splits``, ``pre_ok``.  The launches follow the same plan, so the side buffers are sized from
    it.  Raises where the library has no kernel for the request."""
    k = _KINDS[kind]
    flag = (FPROP_X3, DGRAD_X3, WGRAD_X3)[k] if x3 is None else x3
    plan = ConvPlan()
    check(lib().bdv_conv_plan_query(ctypes.byref(g), k, PIECES if flag else 0, int(pre), ctypes.byref(plan)), 'bdv_conv_plan_query')
    return plan


def _chk_bf16_arith(g: ConvGeom, x3, who: str):
    if g.act_dtype == 1 and not (x3 and PIECES == 1):
        raise ValueError(f"{who}: bf16 tensors need set_conv_arith('bf16') and a geometry of the plane kernels")


def conv_kernel_name(g: ConvGeom, kind: str, x3: Optional[bool] = None) -> str:
    """Name of the main kernel ``conv_fprop`` / ``conv_dgrad`` / ``conv_wgrad(_partial)`` launches for this geometry."""
    return conv_plan(g, kind, x3).kernel.decode()


def conv_uses_planes(g: ConvGeom, kind: str) -> bool:
    """True when ``conv_fprop`` / ``conv_dgrad`` of this geometry read the cached bf16 weight planes (the cache that
    ``bump_weight_epoch`` invalidates) in the current arithmetic."""
    return bool(conv_plan(g, kind).reads_planes)


PRE_BN_1X1_ONLY = _os.environ.get('BDVCIL_PRE_BN_3X3', '0') == '0'


def fprop_pre_ok(g: ConvGeom) -> bool:
    """True when ``conv_fprop(pre_bn=...)`` and ``conv_wgrad*(pre_bn=...)`` can apply the producer's BatchNorm + ReLU in their
    loaders for this geometry (bf16-piece arithmetic with the plane kernels; no temporal shift)."""
    if PRE_BN_1X1_ONLY and (g.R != 1 or g.S != 1):   # a 3x3 consumer re-applies the BatchNorm once per filter tap: measured slower
        return False
    if not (PIECES == 3 and FPROP_X3 and WGRAD_X3 and DGRAD_X3) or g.Rt > 1 or g.act_dtype != 0 or getattr(g, 'frames_view', False):
        return False
    return bool(conv_plan(g, 'fprop').pre_ok and conv_plan(g, 'wgrad').pre_ok)


def conv_fprop(x: torch.Tensor, w: torch.Tensor, g: ConvGeom, out: Optional[torch.Tensor] = None,
               ws_tag: str = 'conv', bn_stats: bool = False, affine=None, x3: Optional[bool] = None, pre_bn=None):
    """x (N,H,W,Cin) NHWC, w (Cout,R,S,Cin) -> y (N,Ho,Wo,Cout); with bn_stats also the fused BatchNorm partial
    sums (float[2][rows][Cout]) for ``bn_train_finalize``.
    ``affine = (scale, shift, residual | None, relu)``: eval-mode BatchNorm folded into the epilogue,
    y = relu?(conv * scale + shift (+ residual)).
    ``pre_bn = (scale, shift)``: x is the RAW output of the producing conv; its train-mode BatchNorm + ReLU is applied in the
    loader (``fprop_pre_ok(g)``), so no apply pass / activation / mask is needed for this consumer."""
    g.act_dtype = _act_code(x)
    _chk_conv(x, (_in_frames(g), g.H, g.W, g.Cin), g, 'x')
    _chk(w, (g.Cout, _taps_r(g), g.S, g.Cin), name='w')
    y = out if out is not None else torch.empty((g.N, g.Ho, g.Wo, g.Cout), dtype=x.dtype, device=x.device)
    _chk_conv(y, (g.N, g.Ho, g.Wo, g.Cout), g, 'y')
    use_x3 = FPROP_X3 if x3 is None else x3
    _chk_bf16_arith(g, use_x3, 'conv_fprop')
    plan = conv_plan(g, 'fprop', use_x3, pre_bn is not None)
    ws = _conv_ws(g, 0, x.device, ws_tag)
    part = aff = None
    if pre_bn is not None:
        _chk(pre_bn[0], (g.Cin,), name='pre_scale')
        _chk(pre_bn[1], (g.Cin,), name='pre_shift')
    if bn_stats:
        if affine is not None:
            raise ValueError('conv_fprop: bn_stats and affine exclude each other')
        part = torch.empty((2, plan.stat_rows, g.Cout), dtype=torch.float32, device=x.device)
    if affine is not None:
        scale, shift, res, relu = affine
        _chk(scale, (g.Cout,), name='scale')
        _chk(shift, (g.Cout,), name='shift')
        if res is not None:
            _chk_conv(res, (g.N, g.Ho, g.Wo, g.Cout), g, 'residual')
        aff = ConvAffine(scale.data_ptr(), shift.data_ptr(), res.data_ptr() if res is not None else None, int(bool(relu)))
    if out is not None:
        amax_forget(out)
    if use_x3 and PIECES == F16X2:
        f16 = _plan_f16(plan)
        planes_f = weight_planes(w, g, f16)[0] if plan.reads_planes else None
        check(lib().bdv_conv_fprop_f16x2(_p(x), _p(act_amax(x) if f16 else None), _p(w), _p(planes_f), _p(y), ctypes.byref(g), _p(part),
                                         ctypes.byref(aff) if aff is not None else None, _p(ws), ws.numel(),
                                         _p(pre_bn[0] if pre_bn is not None else None), _p(pre_bn[1] if pre_bn is not None else None),
                                         _stream()), 'bdv_conv_fprop_f16x2')
    elif use_x3:
        planes_f = weight_planes(w, g)[0] if plan.reads_planes else None
        check(lib().bdv_conv_fprop_pl(_p(x), _p(w), _p(planes_f), _p(y), ctypes.byref(g), _p(part),
                                      ctypes.byref(aff) if aff is not None else None, _p(ws), ws.numel(), PIECES,
                                      _p(pre_bn[0] if pre_bn is not None else None), _p(pre_bn[1] if pre_bn is not None else None),
                                      _stream()), 'bdv_conv_fprop_pl')
    else:
        check(lib().bdv_conv_fprop(_p(x), _p(w), _p(y), ctypes.byref(g), _p(part), ctypes.byref(aff) if aff is not None else None,
                                   _p(ws), ws.numel(), _stream()), 'bdv_conv_fprop')
    return (y, part) if bn_stats else y


DGRAD_X3 = _x3_default('BDVCIL_DGRAD_X3')


def conv_dgrad(dy: torch.Tensor, w: torch.Tensor, g: ConvGeom, add_src: Optional[torch.Tensor] = None,
               add_mask_src: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               ws_tag: str = 'conv', bn_stats=None, x3: Optional[bool] = None):
    """``bn_stats = (y, relu_mask | None, mean, invstd)`` of the conv unit whose output gradient this dgrad produces:
    the BatchNorm-backward statistics are then taken in the epilogue and ``(dx, partial)`` is returned; pass ``partial``
    to ``bn_backward(stat_partial=...)``.  Stride 2 needs a filter that reaches every input pixel (R, S >= 2)."""
    g.act_dtype = _act_code(dy)
    _chk_conv(dy, (g.N, g.Ho, g.Wo, g.Cout), g, 'dy')
    _chk(w, (g.Cout, g.R, g.S, g.Cin), name='w')
    dx = out if out is not None else torch.empty((g.N, g.H, g.W, g.Cin), dtype=dy.dtype, device=dy.device)
    _chk_conv(dx, (g.N, g.H, g.W, g.Cin), g, 'dx')
    if add_src is not None:
        _chk_conv(add_src, (g.N, g.H, g.W, g.Cin), g, 'add_src')
        if add_src.data_ptr() == dx.data_ptr() and g.fold > 0:
            raise ValueError('conv_dgrad: in-place add_src is not allowed with a temporal shift (scatter epilogue)')
    if add_mask_src is not None:
        _chk(add_mask_src, (g.N * g.H * g.W * g.Cin // 32,), dtype=torch.int32, name='add_mask_src')
    use_x3 = DGRAD_X3 if x3 is None else x3
    _chk_bf16_arith(g, use_x3, 'conv_dgrad')
    plan = conv_plan(g, 'dgrad', use_x3)
    fuse = partial = None
    relu_affine = None
    if bn_stats is not None:
        if len(bn_stats) == 5:      # (y, None, mean, invstd, (scale, shift)): the unit's ReLU sign is derived from y
            y, mask, mean, invstd, relu_affine = bn_stats
        else:
            y, mask, mean, invstd = bn_stats
        _chk_conv(y, (g.N, g.H, g.W, g.Cin), g, 'y')
        _chk(mean, (g.Cin,), name='mean')
        _chk(invstd, (g.Cin,), name='invstd')
        if mask is not None:
            _chk(mask, (y.numel() // 32,), dtype=torch.int32, name='relu_mask')
        partial = torch.empty((2, plan.stat_rows, g.Cin), dtype=torch.float32, device=dy.device)
        if relu_affine is not None:
            if mask is not None:
                raise ValueError('conv_dgrad: a ReLU mask and a derived ReLU sign exclude each other')
            _chk(relu_affine[0], (g.Cin,), name='relu_scale')
            _chk(relu_affine[1], (g.Cin,), name='relu_shift')
        fuse = BnStatFuse(y.data_ptr(), mask.data_ptr() if mask is not None else None, mean.data_ptr(), invstd.data_ptr(),
                          partial.data_ptr(), relu_affine[0].data_ptr() if relu_affine is not None else None,
                          relu_affine[1].data_ptr() if relu_affine is not None else None)
    ws = _conv_ws(g, 1, dy.device, ws_tag)
    if out is not None:
        amax_forget(out)
    if use_x3 and PIECES == F16X2:
        f16 = _plan_f16(plan)
        planes_d = weight_planes(w, g, f16)[1] if plan.reads_planes else None
        check(lib().bdv_conv_dgrad_f16x2(_p(dy), _p(act_amax(dy) if f16 else None), _p(w), _p(planes_d), _p(dx), _p(add_src),
                                         _p(add_mask_src), ctypes.byref(g), ctypes.byref(fuse) if fuse is not None else None, _p(ws),
                                         ws.numel(), _stream()), 'bdv_conv_dgrad_f16x2')
    elif use_x3:
        planes_d = weight_planes(w, g)[1] if plan.reads_planes else None
        check(lib().bdv_conv_dgrad_pl(_p(dy), _p(w), _p(planes_d), _p(dx), _p(add_src), _p(add_mask_src), ctypes.byref(g),
                                      ctypes.byref(fuse) if fuse is not None else None, _p(ws), ws.numel(), PIECES, _stream()),
              'bdv_conv_dgrad_pl')
    else:
        check(lib().bdv_conv_dgrad(_p(dy), _p(w), _p(dx), _p(add_src), _p(add_mask_src), ctypes.byref(g),
                                   ctypes.byref(fuse) if fuse is not None else None, _p(ws), ws.numel(), _stream()), 'bdv_conv_dgrad')
    return dx if bn_stats is None else (dx, partial)


def conv_wgrad(dy: torch.Tensor, x: torch.Tensor, g: ConvGeom, dw: Optional[torch.Tensor] = None,
               beta: float = 0.0, ws_tag: str = 'wgrad', x3: Optional[bool] = None, pre_bn=None) -> torch.Tensor:
    """dw = beta * dw + dy^T (*) x in one call (split-K main kernel + fixed-order reduction)."""
    g.act_dtype = _act_code(dy)
    _chk_conv(dy, (g.N, g.Ho, g.Wo, g.Cout), g, 'dy')
    _chk_conv(x, (_in_frames(g), g.H, g.W, g.Cin), g, 'x')
    if dw is None:
        dw = torch.empty((g.Cout, _taps_r(g), g.S, g.Cin), dtype=torch.float32, device=dy.device)
        beta = 0.0
    _chk(dw, (g.Cout, _taps_r(g), g.S, g.Cin), name='dw')
    if WGRAD_X3 if x3 is None else x3:      # the bf16-piece main kernel only exists in the partial + reduce form
        slab, _ = conv_wgrad_partial(dy, x, g, x3=True, dw=dw, pre_bn=pre_bn)
        wgrad_reduce_batched([(slab, dw)], beta=beta)
        return dw
    _chk_bf16_arith(g, False, 'conv_wgrad')
    conv_plan(g, 'wgrad', False, pre_bn is not None)       # refuses pre_bn, temporal taps: the fp32-MFMA kernel has neither
    ws = _conv_ws(g, 2, dy.device, ws_tag)
    check(lib().bdv_conv_wgrad(_p(dy), _p(x), _p(dw), float(beta), ctypes.byref(g), _p(ws), ws.numel(), _stream()),
          'bdv_conv_wgrad')
    return dw


# ---------------------------------------------------------------------------------------------
# batch norm (+ReLU, +residual)
# ---------------------------------------------------------------------------------------------

def _bn_ws(M, C, device):
    return workspace(lib().bdv_bn_workspace_bytes(int(M), int(C)), device, 'bn')


_FIN_SCRATCH = {}   # (device index, stream handle) -> zero-filled scratch + tickets of the split finalize kernels
_FIN_SCRATCH_MIN_C = 2048


def _bn_fin_scratch(C, device):
    """Group sums and tickets of the multi-block finalize kernels (csrc/bn.hip slab_colsum2_split), one set per stream: two
    launches that may overlap (the downsample branch finalizes on the side stream while the main stream finalizes too) must never
    share tickets.  The buffer is zero-filled ONCE, here, and never memset again: the last block to arrive for a channel group
    stores 0 back to its ticket before it exits, kernels of one stream are ordered, and an aborted launch ends the process --
    so every launch finds its tickets zero without a fill launch of the size this split removes."""
    dev = torch.device(device)
    key = (dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    cur = _FIN_SCRATCH.get(key)
    need = lib().bdv_bn_finalize_scratch_bytes(max(int(C), _FIN_SCRATCH_MIN_C))
    if cur is None or cur.numel() < need:
        cur = torch.zeros(need, dtype=torch.uint8, device=dev)
        _FIN_SCRATCH[key] = cur
    return cur


def _bn_fin_args(splits, C, device):
    """(pointer, byte count) of the finalize scratch for a call with ``splits`` blocks per channel group: none for one block."""
    fs = _bn_fin_scratch(C, device) if splits != 1 else None
    return _p(fs), fs.numel() if fs is not None else 0


def _bn_stat_rows(stat_partial, C, who, name='stat_partial'):
    """Checks the ``(2, rows, C)`` tile sums of a ``conv_dgrad(bn_stats=...)`` call -> rows (0 without them)."""
    if stat_partial is None:
        return 0
    _chk(stat_partial, name=name)
    if stat_partial.dim() != 3 or stat_partial.shape[0] != 2 or stat_partial.shape[2] != C:
        raise ValueError(f'{who}: {name} {tuple(stat_partial.shape)} is not (2, rows, {C})')
    return stat_partial.shape[1]


def _bn_param_grads(C, device):
    """Fresh (dgamma, dbeta)."""
    return torch.empty(C, dtype=torch.float32, device=device), torch.empty(C, dtype=torch.float32, device=device)


def bn_train_stats(y, gamma, beta, eps, momentum, running_mean, running_var):
    """y (..., C) -> (save_mean, save_invstd, scale, shift); running stats updated in place."""
    C = y.shape[-1]
    M = y.numel() // C
    _chk(y, name='y')
    for t, n in ((gamma, 'gamma'), (beta, 'beta')):
        _chk(t, (C,), name=n)
    if running_mean is not None:
        _chk(running_mean, (C,), name='running_mean')
        _chk(running_var, (C,), name='running_var')
    stats = torch.empty((4, C), dtype=torch.float32, device=y.device)
    ws = _bn_ws(M, C, y.device)
    check(lib().bdv_bn_train_stats(_p(y), M, C, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
                                   _p(running_var), _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(ws),
                                   ws.numel(), _stream()), 'bdv_bn_train_stats')
    return stats[0], stats[1], stats[2], stats[3]


def bn_train_finalize(partial, M, gamma, beta, eps, momentum, running_mean, running_var, splits=0):
    """partial float[2][rows][C] from conv_fprop(bn_stats=True) -> (save_mean, save_invstd, scale, shift).
    ``splits``: blocks per channel group of the finalize kernel (0 = the library's rule, 1 = one block; same bits either way)."""
    _chk(partial, name='partial')
    _, rows, C = partial.shape
    for t, n in ((gamma, 'gamma'), (beta, 'beta')):
        _chk(t, (C,), name=n)
    if running_mean is not None:
        _chk(running_mean, (C,), name='running_mean')
        _chk(running_var, (C,), name='running_var')
    stats = torch.empty((4, C), dtype=torch.float32, device=partial.device)
    check(lib().bdv_bn_train_finalize_split(_p(partial), rows, int(M), C, _p(gamma), _p(beta), float(eps), float(momentum),
                                            _p(running_mean), _p(running_var), _p(stats[0]), _p(stats[1]), _p(stats[2]),
                                            _p(stats[3]), int(splits), *_bn_fin_args(splits, C, partial.device), _stream()),
          'bdv_bn_train_finalize_split')
    return stats[0], stats[1], stats[2], stats[3]


def bn_eval_params(gamma, beta, running_mean, running_var, eps):
    C = gamma.numel()
    for t, n in ((gamma, 'gamma'), (beta, 'beta'), (running_mean, 'running_mean'), (running_var, 'running_var')):
        _chk(t, (C,), name=n)
    ss = torch.empty((2, C), dtype=torch.float32, device=gamma.device)
    check(lib().bdv_bn_eval_params(C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps), _p(ss[0]),
                                   _p(ss[1]), _stream()), 'bdv_bn_eval_params')
    return ss[0], ss[1]


def bn_apply(y, scale, shift, res=None, relu=True, out=None, want_mask=False, res_affine=None):
    """-> out, or (out, relu_mask) when want_mask (int32 tensor, 1 bit per element: out > 0).
    ``res_affine = (scale, shift)``: the residual is a raw conv output and gets its own BatchNorm here."""
    C = y.shape[-1]
    M = y.numel() // C
    _chk_act(y, name='y')
    _chk(scale, (C,), name='scale')
    _chk(shift, (C,), name='shift')
    if res is not None:
        _chk_act(res, tuple(y.shape), name='res', like=y)
    rs = rb = None
    if res_affine is not None:
        if res is None:
            raise ValueError('bn_apply: res_affine needs res')
        rs, rb = res_affine
        _chk(rs, (C,), name='res_scale')
        _chk(rb, (C,), name='res_shift')
    o = out if out is not None else torch.empty_like(y)
    _chk_act(o, tuple(y.shape), name='out', like=y)
    amax_forget(out)
    mask = None
    if want_mask:
        if not relu or C % 32 != 0:
            raise ValueError('bn_apply: a ReLU mask needs relu=True and C % 32 == 0')
        mask = torch.empty(y.numel() // 32, dtype=torch.int32, device=y.device)
    check(lib().bdv_bn_apply(_p(y), _p(scale), _p(shift), _p(res), _p(rs), _p(rb), _p(o), _p(mask), M, C, int(bool(relu)),
                             _act_code(y), _stream()), 'bdv_bn_apply')
    return (o, mask) if want_mask else o


def bn_backward(dout, relu_mask, y, gamma, save_mean, save_invstd, relu, dgamma=None, dbeta=None, beta_acc=0.0, dy=None,
                stat_partial=None, relu_affine=None, splits=0):
    """Returns (dy, dgamma, dbeta).  ``relu_mask`` is the bit mask from ``bn_apply(want_mask=True)`` (needed when relu), or None
    with ``relu_affine = (scale, shift)``: the sign is then derived from y (a unit whose apply pass never ran).
    ``stat_partial``: the ``(2, rows, C)`` tile sums from ``conv_dgrad(bn_stats=...)``; the statistics pass is skipped.
    ``splits``: as ``bn_train_finalize``."""
    C = y.shape[-1]
    M = y.numel() // C
    _chk_act(y, name='y')
    _chk_act(dout, tuple(y.shape), name='dout', like=y)
    if relu and relu_affine is None:
        _chk(relu_mask, (y.numel() // 32,), dtype=torch.int32, name='relu_mask')
    if relu_affine is not None:
        if not relu or relu_mask is not None:
            raise ValueError('bn_backward: relu_affine goes with relu=True and relu_mask=None')
        _chk(relu_affine[0], (C,), name='relu_scale')
        _chk(relu_affine[1], (C,), name='relu_shift')
    for t, n in ((gamma, 'gamma'), (save_mean, 'save_mean'), (save_invstd, 'save_invstd')):
        _chk(t, (C,), name=n)
    if dgamma is None:
        dgamma, dbeta = _bn_param_grads(C, y.device)
        beta_acc = 0.0
    _chk(dgamma, (C,), name='dgamma')
    _chk(dbeta, (C,), name='dbeta')
    d = dy if dy is not None else torch.empty_like(y)
    _chk_act(d, tuple(y.shape), name='dy', like=y)
    amax_forget(dy)
    srows = _bn_stat_rows(stat_partial, C, 'bn_backward')
    ws = _bn_ws(M, C, y.device)
    check(lib().bdv_bn_backward_split(_p(dout), _p(relu_mask if relu else None), _p(y), _p(gamma), _p(save_mean), _p(save_invstd),
                                      _p(d), _p(dgamma), _p(dbeta), float(beta_acc), M, C, int(bool(relu)), _p(stat_partial), srows,
                                      _p(relu_affine[0] if relu_affine is not None else None),
                                      _p(relu_affine[1] if relu_affine is not None else None), _p(ws), ws.numel(), _act_code(y),
                                      int(splits), *_bn_fin_args(splits, C, y.device), _stream()), 'bdv_bn_backward_split')
    return d, dgamma, dbeta


def bn_backward_pair(dout, relu_mask, ya, gamma_a, mean_a, invstd_a, yb, gamma_b, mean_b, invstd_b, stat_partial_a=None, splits=0):
    """Backward of the two BatchNorms behind one masked gradient ``dout * relu_mask`` (a block with a downsample branch: ``a`` = its
    last main unit, ``b`` = the downsample BatchNorm) -> ((dya, dgamma_a, dbeta_a), (dyb, dgamma_b, dbeta_b)), bit-identical to
    two ``bn_backward(..., relu=True)`` calls; ``dout`` and the mask are read once per pass.  ``stat_partial_a``: as
    ``bn_backward(stat_partial=...)`` for ``a``."""
    C = ya.shape[-1]
    M = ya.numel() // C
    _chk_act(ya, name='ya')
    _chk_act(yb, tuple(ya.shape), name='yb', like=ya)
    _chk_act(dout, tuple(ya.shape), name='dout', like=ya)
    if C % 32 != 0:
        raise ValueError('bn_backward_pair: C % 32 != 0')
    _chk(relu_mask, (ya.numel() // 32,), dtype=torch.int32, name='relu_mask')
    for t, n in ((gamma_a, 'gamma_a'), (mean_a, 'mean_a'), (invstd_a, 'invstd_a'), (gamma_b, 'gamma_b'), (mean_b, 'mean_b'),
                 (invstd_b, 'invstd_b')):
        _chk(t, (C,), name=n)
    srows = _bn_stat_rows(stat_partial_a, C, 'bn_backward_pair', 'stat_partial_a')
    dya, dyb = torch.empty_like(ya), torch.empty_like(yb)
    pg = _bn_param_grads(C, ya.device) + _bn_param_grads(C, ya.device)      # dgamma_a, dbeta_a, dgamma_b, dbeta_b
    ws = workspace(lib().bdv_bn_pair_workspace_bytes(M, C), ya.device, 'bn')
    check(lib().bdv_bn_backward_pair(_p(dout), _p(relu_mask), _p(ya), _p(gamma_a), _p(mean_a), _p(invstd_a), _p(stat_partial_a), srows,
                                     _p(dya), _p(pg[0]), _p(pg[1]), _p(yb), _p(gamma_b), _p(mean_b), _p(invstd_b), _p(dyb), _p(pg[2]),
                                     _p(pg[3]), M, C, _p(ws), ws.numel(), _act_code(ya), int(splits), *_bn_fin_args(splits, C, ya.device),
                                     _stream()), 'bdv_bn_backward_pair')
    return (dya, pg[0], pg[1]), (dyb, pg[2], pg[3])


_BN_UNIT = {}       # (device, C) -> (ones, zeros): the identity affine


def bn_unit_affine(C, device):
    """(ones, zeros) of C channels on ``device``, cached: gamma / beta (or scale / shift) of an identity BatchNorm."""
    key = (device.type, device.index or 0, C)
    unit = _BN_UNIT.get(key)
    if unit is None:
        unit = _BN_UNIT[key] = (torch.ones(C, dtype=torch.float32, device=device), torch.zeros(C, dtype=torch.float32, device=device))
    return unit


def bn_eval_invstd(running_var, eps):
    """1 / sqrt(running_var + eps) as ``bn_eval_params`` rounds it (scale for gamma = 1): the invstd of an eval-mode BatchNorm."""
    one, zero = bn_unit_affine(running_var.numel(), running_var.device)
    return bn_eval_params(one, zero, zero, running_var, eps)[0]


def bn_eval_backward(dout, scale, relu_mask=None, relu_act=None, y=None, running_mean=None, invstd=None, want_params=False,
                     want_dz=False, dgamma=None, dbeta=None, beta_acc=0.0, dy=None, splits=0):
    """Backward through an eval-mode BatchNorm (+ ReLU) -> (dy, dz | None, dgamma | None, dbeta | None).
    ``scale`` = gamma * invstd_running (``bn_eval_params``); dz = dout * sign, dy = dz * scale.  Sign: ``relu_mask`` (the bits of
    ``bn_apply(want_mask=True)``), or ``relu_act`` (an activation: act > 0), or neither (no ReLU).  ``want_params`` (or ``dgamma`` /
    ``dbeta`` to accumulate into with ``beta_acc``): also dbeta = sum dz, dgamma = sum dz * (y - running_mean) * invstd, which needs
    ``y``, ``running_mean`` and ``invstd``; without it none of the three is read.  ``splits``: as ``bn_train_finalize``."""
    C = dout.shape[-1]
    M = dout.numel() // C
    _chk_act(dout, name='dout')
    _chk(scale, (C,), name='scale')
    if relu_mask is not None and relu_act is not None:
        raise ValueError('bn_eval_backward: relu_mask and relu_act are two sources of the same sign: give one')
    if relu_mask is not None:
        if C % 32 != 0:
            raise ValueError('bn_eval_backward: a ReLU mask needs C % 32 == 0')
        _chk(relu_mask, (dout.numel() // 32,), dtype=torch.int32, name='relu_mask')
    if relu_act is not None:
        _chk_act(relu_act, tuple(dout.shape), name='relu_act', like=dout)
    params = want_params or dgamma is not None or dbeta is not None
    ws = None
    if params:
        if y is None or running_mean is None or invstd is None:
            raise ValueError('bn_eval_backward: parameter gradients need y, running_mean and invstd')
        _chk_act(y, tuple(dout.shape), name='y', like=dout)
        _chk(running_mean, (C,), name='running_mean')
        _chk(invstd, (C,), name='invstd')
        if (dgamma is None) != (dbeta is None):
            raise ValueError('bn_eval_backward: give dgamma and dbeta together (to accumulate into) or neither')
        if dgamma is None:
            dgamma, dbeta = _bn_param_grads(C, dout.device)
            beta_acc = 0.0
        _chk(dgamma, (C,), name='dgamma')
        _chk(dbeta, (C,), name='dbeta')
        ws = _bn_ws(M, C, dout.device)
    else:
        y = running_mean = invstd = None
    d = dy if dy is not None else torch.empty_like(dout)
    _chk_act(d, tuple(dout.shape), name='dy', like=dout)
    dz = torch.empty_like(dout) if want_dz else None
    check(lib().bdv_bn_eval_backward(_p(dout), _p(relu_mask), _p(relu_act), _p(y), _p(scale), _p(running_mean), _p(invstd), _p(d),
                                     _p(dz), _p(dgamma), _p(dbeta), float(beta_acc), M, C, _p(ws), ws.numel() if ws is not None else 0,
                                     _act_code(dout), int(splits), *(_bn_fin_args(splits, C, dout.device) if params else (None, 0)),
                                     _stream()), 'bdv_bn_eval_backward')
    return d, dz, dgamma, dbeta


def bn_backward_maxpool(dpool, pool_idx, relu_mask, y, gamma, save_mean, save_invstd, splits=0):
    """BN(+ReLU) backward behind MaxPool2d(3,2,1) (the stem): the pooled gradient is expanded on the fly.
    -> (dy, dgamma, dbeta)."""
    _chk(y, name='y')
    N, H, W, C = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _chk_act(dpool, (N, Ho, Wo, C), name='dpool')      # the pooled tensor's gradient carries the activation storage type; y / dy are fp32
    _chk(pool_idx, (N, Ho, Wo, C), dtype=torch.uint8, name='pool_idx')
    _chk(relu_mask, (y.numel() // 32,), dtype=torch.int32, name='relu_mask')
    for t, n in ((gamma, 'gamma'), (save_mean, 'save_mean'), (save_invstd, 'save_invstd')):
        _chk(t, (C,), name=n)
    dy = torch.empty_like(y)
    dgamma, dbeta = _bn_param_grads(C, y.device)
    ws = _bn_ws(N * H * W, C, y.device)
    check(lib().bdv_bn_backward_maxpool_split(_p(dpool), _p(pool_idx), _p(relu_mask), _p(y), _p(gamma), _p(save_mean), _p(save_invstd),
                                              _p(dy), _p(dgamma), _p(dbeta), 0.0, N, H, W, C, _p(ws), ws.numel(), _act_code(dpool),
                                              int(splits), *_bn_fin_args(splits, C, y.device), _stream()),
          'bdv_bn_backward_maxpool_split')
    return dy, dgamma, dbeta


def relu_bwd(dout, relu_mask, add=None, g=None):
    _chk_act(dout, name='dout')
    _chk(relu_mask, (dout.numel() // 32,), dtype=torch.int32, name='relu_mask')
    if add is not None:
        _chk_act(add, tuple(dout.shape), name='add', like=dout)
    r = g if g is not None else torch.empty_like(dout)
    _chk_act(r, tuple(dout.shape), name='g', like=dout)
    check(lib().bdv_relu_bwd(_p(dout), _p(relu_mask), _p(add), _p(r), dout.numel(), _act_code(dout), _stream()), 'bdv_relu_bwd')
    return r


def add(a, b, out=None):
    _chk_act(a, name='a')
    _chk_act(b, tuple(a.shape), name='b', like=a)
    o = out if out is not None else torch.empty_like(a)
    _chk_act(o, tuple(a.shape), name='out', like=a)
    amax_forget(out)
    check(lib().bdv_add(_p(a), _p(b), _p(o), a.numel(), _act_code(a), _stream()), 'bdv_add')
    return o


# ---------------------------------------------------------------------------------------------
# stem helpers / pooling / front-end
# ---------------------------------------------------------------------------------------------

def nchw3_to_nhwc4(x):
    """(N,3,H,W) -> (N,H,W,4)."""
    _chk(x, name='x')
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f'nchw3_to_nhwc4: expected (N,3,H,W), got {tuple(x.shape)}')
    N, _, H, W = x.shape
    out = torch.empty((N, H, W, 4), dtype=torch.float32, device=x.device)
    check(lib().bdv_nchw3_to_nhwc4(_p(x), _p(out), N, H, W, _stream()), 'bdv_nchw3_to_nhwc4')
    return out


def maxpool_fwd(x, out_dtype=torch.float32):
    """``out_dtype``: ``ACT_DTYPE`` at the 2-D stem (the pooled tensor is the first one in the activation storage type)."""
    _chk(x, name='x')
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, Ho, Wo, C), dtype=out_dtype, device=x.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    check(lib().bdv_maxpool_fwd(_p(x), _p(out), _p(idx), N, H, W, C, _act_code(out), _stream()), 'bdv_maxpool_fwd')
    return out, idx


def bn_relu_maxpool_fwd(y, scale, shift, out_dtype=torch.float32):
    """Stem tail: relu(y * scale + shift) -> MaxPool2d(3,2,1) in one pass -> (pooled, idx, relu_mask of the activation)."""
    _chk(y, name='y')
    N, H, W, C = y.shape
    _chk(scale, (C,), name='scale')
    _chk(shift, (C,), name='shift')
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, Ho, Wo, C), dtype=out_dtype, device=y.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=y.device)
    mask = torch.empty(y.numel() // 32, dtype=torch.int32, device=y.device)
    check(lib().bdv_bn_relu_maxpool_fwd(_p(y), _p(scale), _p(shift), _p(out), _p(idx), _p(mask), N, H, W, C, _act_code(out), _stream()),
          'bdv_bn_relu_maxpool_fwd')
    return out, idx, mask


def maxpool_t2_fwd(x):
    """MaxPool3d((2,1,1),(2,1,1)) on frames (2n, H, W, C) -> ((n, H, W, C), sel bit mask).  The output has x's storage type."""
    _chk_act(x, name='x')
    N2, H, W, C = x.shape
    if N2 % 2 or (H * W * C) % 32:
        raise ValueError(f'maxpool_t2_fwd: {tuple(x.shape)}: needs an even frame count and H*W*C % 32 == 0')
    out = torch.empty((N2 // 2, H, W, C), dtype=x.dtype, device=x.device)
    sel = torch.empty(out.numel() // 32, dtype=torch.int32, device=x.device)
    check(lib().bdv_maxpool_t2_fwd_act(_p(x), _p(out), _p(sel), N2 // 2, H * W * C, _act_code(x), _stream()), 'bdv_maxpool_t2_fwd_act')
    return out, sel


def maxpool_t2_bwd(dout, sel):
    """-> dx (2n, H, W, C) in dout's storage type: the gradient at the frame ``sel`` names, zero at the other one."""
    _chk_act(dout, name='dout')
    n, H, W, C = dout.shape
    _chk(sel, (dout.numel() // 32,), dtype=torch.int32, name='sel')
    dx = torch.empty((2 * n, H, W, C), dtype=dout.dtype, device=dout.device)
    check(lib().bdv_maxpool_t2_bwd_act(_p(dout), _p(sel), _p(dx), n, H * W * C, _act_code(dout), _stream()), 'bdv_maxpool_t2_bwd_act')
    return dx


def maxpool_bwd(dout, idx, in_shape):
    N, H, W, C = in_shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _chk_act(dout, (N, Ho, Wo, C), name='dout')
    _chk(idx, (N, Ho, Wo, C), dtype=torch.uint8, name='idx')
    dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dout.device)
    check(lib().bdv_maxpool_bwd(_p(dout), _p(idx), _p(dx), N, H, W, C, _act_code(dout), _stream()), 'bdv_maxpool_bwd')
    return dx


def avgpool_fwd(x):
    _chk_act(x, name='x')
    N, H, W, C = x.shape
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(lib().bdv_avgpool_fwd(_p(x), _p(out), N, H * W, C, _act_code(x), _stream()), 'bdv_avgpool_fwd')
    return out


def avgpool_bwd(dout, in_shape, dtype=torch.float32):
    """``dtype``: storage type of the pooled tensor's input (its gradient is written in it)."""
    N, H, W, C = in_shape
    _chk(dout, (N, C), name='dout')
    dx = torch.empty((N, H, W, C), dtype=dtype, device=dout.device)
    check(lib().bdv_avgpool_bwd(_p(dout), _p(dx), N, H * W, C, _act_code(dx), _stream()), 'bdv_avgpool_bwd')
    return dx


def _f3(values):
    return (ctypes.c_float * 3)(*[float(v) for v in values])


def _mean_inv_std(mean, std):
    """``(mean, 1 / std)`` as ``c_float * 3`` each; the reciprocal is taken in fp32, as the CPU restatement computes it."""
    inv = 1.0 / torch.tensor(list(std), dtype=torch.float32)
    return _f3(mean), _f3(inv.tolist())


def _out_pair(B, F, h, w, want_nhwc4, want_nchw, device):
    """The front-ends' outputs for B samples of F frames: ``(o4 (B*F, h, w, 4) | None, oc (B, F, 3, h, w) | None)`` fp32."""
    o4 = torch.empty((B * F, h, w, 4), dtype=torch.float32, device=device) if want_nhwc4 else None
    oc = torch.empty((B, F, 3, h, w), dtype=torch.float32, device=device) if want_nchw else None
    return o4, oc


def _video_runs(counts, device):
    """Frames per video -> ``(first, counts)`` of the videos' runs in a tensor that holds them back to back, as
    ``(first_h int64, counts_h int32, first_d, counts_d)``: on the host (the library validates them there) and on the device."""
    counts_h = torch.tensor([int(c) for c in counts], dtype=torch.int32)
    first_h = torch.zeros(counts_h.shape[0], dtype=torch.int64)
    first_h[1:] = torch.cumsum(counts_h[:-1], 0)
    return first_h, counts_h, first_h.to(device), counts_h.to(device)


def bgmix_normalize_u8(frames, bg, mix, alpha, mean, std, want_nhwc4=True, want_nchw=False):
    """frames (B,T,H,W,3) u8, bg (B,H,W,3) u8 -- or fp32 pixel values in [0,255], the output of ``bg_resize_crop_u8`` -- | None,
    mix (B,) u8/bool | None."""
    _chk(frames, dtype=torch.uint8, name='frames')
    B, T, H, W, c3 = frames.shape
    if c3 != 3:
        raise ValueError('frames must be (B,T,H,W,3)')
    bg_f32 = bg is not None and bg.dtype == torch.float32
    if bg is not None:
        _chk(bg, (B, H, W, 3), dtype=torch.float32 if bg_f32 else torch.uint8, name='bg')
        mix = mix.to(torch.uint8) if mix.dtype != torch.uint8 else mix
        _chk(mix, (B,), dtype=torch.uint8, name='mix')
    else:
        mix = None
    m3, inv3 = _mean_inv_std(mean, std)
    o4, oc = _out_pair(B, T, H, W, want_nhwc4, want_nchw, frames.device)
    check(lib().bdv_bgmix_normalize_u8(_p(frames), _p(bg), int(bg_f32), _p(mix), float(alpha), m3, _f3(std), inv3, _p(o4), _p(oc), B, T, H, W,
                                       _stream()), 'bdv_bgmix_normalize_u8')
    return o4, oc


def resized_size(h: int, w: int, size: int):
    """Output size of torchvision's ``Resize(size)`` with an int: the smaller edge becomes ``size``, the other one
    ``int(size * long / short)`` (UPSTREAM torchvision ``_compute_resized_output_size``)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def bg_resize_crop_u8(bg, size, crop_h, crop_w, top, left):
    """bg (B,Hs,Ws,3) u8 -> (B,crop_h,crop_w,3) fp32 in [0,255]: ``Resize(size)`` + crop at (top[b], left[b]) of
    BackgroundMixDataset.bg_pipeline (libs/loader/comix_loader.py:72-73); top / left: (B,) int32 tensors on the device."""
    _chk(bg, dtype=torch.uint8, name='bg')
    if bg.dim() != 4 or bg.shape[-1] != 3:
        raise ValueError(f'bg_resize_crop_u8: expected (B,Hs,Ws,3), got {tuple(bg.shape)}')
    B, Hs, Ws, _ = bg.shape
    Hr, Wr = resized_size(Hs, Ws, int(size))
    if crop_h > Hr or crop_w > Wr:
        raise ValueError(f'Required crop size {(crop_h, crop_w)} is larger than input image size {(Hr, Wr)}')     # torchvision's message
    _chk(top, (B,), dtype=torch.int32, name='top')
    _chk(left, (B,), dtype=torch.int32, name='left')
    out = torch.empty((B, crop_h, crop_w, 3), dtype=torch.float32, device=bg.device)
    check(lib().bdv_bg_resize_crop_u8(_p(bg), B, Hs, Ws, Hr, Wr, _p(top), _p(left), int(crop_h), int(crop_w), _p(out), _stream()),
          'bdv_bg_resize_crop_u8')
    return out


def resized_crop_f32(frames, boxes, out_h: int, out_w: int, antialias: bool = False):
    """frames (F,H,W,3) u8 on the device; boxes (F,4) int32 ``[top, left, h, w]`` (host array / tensor) -> (F,out_h,out_w,3) fp32:
    each frame's box resized as ``F.interpolate(mode='bilinear', align_corners=False, antialias=antialias)`` resizes the float crop
    (torchvision's ``resized_crop`` of sim_cam_motion_bg_extract, cil_tools/extract_background.py:82)."""
    _chk(frames, dtype=torch.uint8, name='frames')
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'resized_crop_f32: expected (F,H,W,3), got {tuple(frames.shape)}')
    F, H, W, _ = frames.shape
    hb = torch.as_tensor(boxes).to('cpu', torch.int32).reshape(-1, 4).contiguous()
    if hb.shape[0] != F:
        raise ValueError(f'resized_crop_f32: {hb.shape[0]} boxes for {F} frames')
    out = torch.empty((F, int(out_h), int(out_w), 3), dtype=torch.float32, device=frames.device)
    db = hb.to(frames.device)
    check(lib().bdv_resized_crop_f32(_p(frames), F, H, W, _p(db), hb.data_ptr(), int(out_h), int(out_w),
                                     1 if antialias else 0, _p(out), _stream()), 'bdv_resized_crop_f32')
    return out


def temporal_nanreduce_f32(frames, counts, mode: int = 0, zero_is_missing: bool = True):
    """frames (sum(counts), ...) fp32 on the device, the videos' frames back to back; counts: frames per video -> (V, ...) uint8:
    ``np.nanmedian`` (mode 0) / ``np.nanmean`` (mode 1) over each video's frames, ``.astype(np.uint8)``; NaN, and 0 when
    ``zero_is_missing``, count as missing (cil_tools/extract_background.py:92-98)."""
    _chk(frames, dtype=torch.float32, name='frames')
    if frames.dim() < 2:
        raise ValueError(f'temporal_nanreduce_f32: expected (F, ...), got {tuple(frames.shape)}')
    dev = frames.device
    first_h, counts_h, first_d, counts_d = _video_runs(counts, dev)
    V = int(counts_h.shape[0])
    P = 1
    for d in frames.shape[1:]:
        P *= int(d)
    out = torch.empty((V,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=dev)
    check(lib().bdv_temporal_nanreduce_f32(_p(frames), int(frames.shape[0]), _p(first_d), _p(counts_d), first_h.data_ptr(),
                                           counts_h.data_ptr(), V, P, int(mode), 1 if zero_is_missing else 0, _p(out), _stream()),
          'bdv_temporal_nanreduce_f32')
    return out


def temporal_masked_median_u8(frames, counts, box_first, boxes, min_visible: int = 1):
    """frames (sum(counts), H, W, 3) u8 on the device, the videos' frames back to back; counts: frames per video; box_first
    (sum(counts) + 1,) / boxes (nb, 4) int32 host arrays or tensors: the CSR table of half-open person boxes ``x0, y0, x1, y1`` per
    frame -> ``(out (V, H, W, 3) uint8, visible (V, H, W) uint16)``: the median over the frames in which no box covers the pixel, the
    plain median where fewer than ``min_visible`` such frames exist, and their number (the detector-free stand-in for
    cil_tools/type_b_and_c_bg.py:47-54)."""
    _chk(frames, dtype=torch.uint8, name='frames')
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'temporal_masked_median_u8: expected (F,H,W,3), got {tuple(frames.shape)}')
    dev = frames.device
    first_h, counts_h, first_d, counts_d = _video_runs(counts, dev)
    V, H, W = int(counts_h.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    bf_h = torch.as_tensor(box_first).to('cpu', torch.int32).reshape(-1).contiguous()
    bx_h = torch.as_tensor(boxes).to('cpu', torch.int32).reshape(-1, 4).contiguous()
    if bf_h.shape[0] != frames.shape[0] + 1:
        raise ValueError(f'temporal_masked_median_u8: box_first has {bf_h.shape[0]} entries for {frames.shape[0]} frames')
    out = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    visible = torch.empty((V, H, W), dtype=torch.uint16, device=dev)
    bf_d, bx_d = bf_h.to(dev), bx_h.to(dev)
    nb = int(bx_h.shape[0])
    check(lib().bdv_temporal_masked_median_u8(_p(frames), int(frames.shape[0]), _p(first_d), _p(counts_d), first_h.data_ptr(),
                                              counts_h.data_ptr(), V, H, W, _p(bf_d), _p(bx_d) if nb else None, bf_h.data_ptr(),
                                              bx_h.data_ptr() if nb else None, nb, int(min_visible), _p(out), _p(visible), _stream()),
          'bdv_temporal_masked_median_u8')
    return out, visible


def resize_linear_u8(frames, Hd: int, Wd: int, boxes=None):
    """``cv2.resize(..., INTER_LINEAR)`` of uint8 frames (.., Hs, Ws, 3) -> (.., Hd, Wd, 3).  ``boxes``: None, or for frames of shape
    (B, T, Hs, Ws, 3) a list / (B, 4) array of per-clip crops (x0, y0, w, h) that are cut out and resized in the same pass
    (MultiScaleCrop + Resize)."""
    _chk(frames, dtype=torch.uint8, name='frames')
    if frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError(f'resize_linear_u8: expected (..., H, W, 3), got {tuple(frames.shape)}')
    Hs, Ws = int(frames.shape[-3]), int(frames.shape[-2])
    lead = tuple(frames.shape[:-3])
    N = 1
    for d in lead:
        N *= int(d)
    out = torch.empty(lead + (int(Hd), int(Wd), 3), dtype=torch.uint8, device=frames.device)
    dev_boxes, host_boxes, per = None, None, 1
    if boxes is not None:
        if frames.dim() != 5:
            raise ValueError('resize_linear_u8: per-clip boxes need frames of shape (B, T, H, W, 3)')
        hb = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 4).contiguous()
        if hb.shape[0] != frames.shape[0]:
            raise ValueError(f'resize_linear_u8: {hb.shape[0]} boxes for {frames.shape[0]} clips')
        host_boxes, dev_boxes, per = hb, hb.to(frames.device), int(frames.shape[1])
    check(lib().bdv_resize_linear_u8(_p(frames), N, Hs, Ws, _p(dev_boxes), per, host_boxes.data_ptr() if host_boxes is not None else None,
                                     _p(out), int(Hd), int(Wd), _stream()), 'bdv_resize_linear_u8')
    return out


def crop_normalize_u8(frames, crops, crop_h, crop_w, mean, std, want_nhwc4=True, want_nchw=False):
    """frames (B,T,H,W,3) u8; crops = [(x_offset, y_offset, flip), ...] -> (o4 (B*n*T, ch, cw, 4) | None,
    oc (B, n*T, 3, ch, cw) | None), crop-major frame order."""
    _chk(frames, dtype=torch.uint8, name='frames')
    if frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError('frames must be (B,T,H,W,3)')
    B, T, H, W, _ = frames.shape
    n = len(crops)
    table = (ctypes.c_int32 * (3 * n))(*[int(v) for c in crops for v in c])
    m3, inv3 = _mean_inv_std(mean, std)
    o4, oc = _out_pair(B, n * T, crop_h, crop_w, want_nhwc4, want_nchw, frames.device)
    check(lib().bdv_crop_normalize_u8(_p(frames), ctypes.cast(table, ctypes.c_void_p), n, int(crop_h), int(crop_w), m3, inv3, _p(o4), _p(oc),
                                      B, T, H, W, _stream()), 'bdv_crop_normalize_u8')
    return o4, oc


def _host_table(table, cols: int, dtype, name: str) -> torch.Tensor:
    t = torch.as_tensor(table, dtype=dtype).contiguous()
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f'{name}: expected a (clips, {cols}) table, got {tuple(t.shape)}')
    return t


def resize_linear_ragged_u8(src, table, T: int, dst):
    """``bdv_resize_linear_ragged_u8``: ``cv2.resize(..., INTER_LINEAR)`` of clips of different sizes in one launch.  ``src`` / ``dst``:
    contiguous uint8 device tensors (a packed buffer of ``decode.RaggedClips``, or the uniform (B, T, S, S, 3) tensor); ``table``: host
    (clips, 10) int64 rows (source byte offset, Hs, Ws, x0, y0, w, h, destination byte offset, Hd, Wd) as ``decode.plan_resize_stage``
    writes them, validated by the library before the launch.  Returns ``dst``."""
    _chk(src, dtype=torch.uint8, name='src')
    _chk(dst, dtype=torch.uint8, name='dst')
    host = _host_table(table, 10, torch.int64, 'resize_linear_ragged_u8')
    dev = host.to(src.device)
    check(lib().bdv_resize_linear_ragged_u8(_p(src), src.numel(), _p(dev), host.data_ptr(), int(host.shape[0]), int(T), _p(dst), dst.numel(),
                                            _stream()), 'bdv_resize_linear_ragged_u8')
    return dst


def crop_normalize_ragged_u8(src, clips, T: int, crops, crop_h, crop_w, mean, std, want_nhwc4=True, want_nchw=False):
    """``crop_normalize_u8`` for clips of different sizes in a packed uint8 buffer ``src``: ``clips`` host (B, 3) int64 rows (byte
    offset, H, W); ``crops`` (B, n, 3): per clip [(x_offset, y_offset, flip), ...] -> (o4 (B*n*T, ch, cw, 4) | None,
    oc (B, n*T, 3, ch, cw) | None), crop-major frame order."""
    _chk(src, dtype=torch.uint8, name='src')
    hc = _host_table(clips, 3, torch.int64, 'crop_normalize_ragged_u8')
    B = int(hc.shape[0])
    hk = torch.as_tensor(crops, dtype=torch.int32).contiguous()
    if hk.dim() != 3 or hk.shape[0] != B or hk.shape[2] != 3:
        raise ValueError(f'crop_normalize_ragged_u8: crops must be ({B}, n, 3), got {tuple(hk.shape)}')
    n = int(hk.shape[1])
    m3, inv3 = _mean_inv_std(mean, std)
    o4, oc = _out_pair(B, n * T, crop_h, crop_w, want_nhwc4, want_nchw, src.device)
    dc, dk = hc.to(src.device), hk.to(src.device)
    check(lib().bdv_crop_normalize_ragged_u8(_p(src), src.numel(), _p(dc), hc.data_ptr(), _p(dk), hk.data_ptr(), n, int(crop_h), int(crop_w),
                                             m3, inv3, _p(o4), _p(oc), B, int(T), _stream()), 'bdv_crop_normalize_ragged_u8')
    return o4, oc


def actor_cut_mix_u8(actor, scene, plan, nclips: int, out, mean, std):
    """ActorCutMix composite + Normalize (``bdv_actor_cut_mix_u8``): actor (n_actor, T, Ha, Wa, 3) / scene (n_scene, T, Hs, Ws, 3) | None
    uint8 clips after Resize(-1, 256); ``plan``: the host int32 table of include/bdvcil_hip.h (validated there before the launch);
    out (B_out, T, 3, Hd, Wd) fp32, the clips' rows written.  Returns the mask pixel counts (nclips,) int32 on the device."""
    _chk(actor, dtype=torch.uint8, name='actor')
    if actor.dim() != 5 or actor.shape[-1] != 3:
        raise ValueError(f'actor_cut_mix_u8: actor must be (n, T, H, W, 3), got {tuple(actor.shape)}')
    n_actor, T, Ha, Wa, _ = (int(d) for d in actor.shape)
    n_scene, Hs, Ws = 0, 0, 0
    if scene is not None:
        _chk(scene, dtype=torch.uint8, name='scene')
        if scene.dim() != 5 or tuple(scene.shape[1:2]) != (T,) or scene.shape[-1] != 3:
            raise ValueError(f'actor_cut_mix_u8: scene must be (n, {T}, H, W, 3), got {tuple(scene.shape)}')
        n_scene, _, Hs, Ws, _ = (int(d) for d in scene.shape)
    _chk(out, dtype=torch.float32, name='out')
    if out.dim() != 5 or out.shape[1] != T or out.shape[2] != 3:
        raise ValueError(f'actor_cut_mix_u8: out must be (B, {T}, 3, Hd, Wd), got {tuple(out.shape)}')
    B_out, Hd, Wd = int(out.shape[0]), int(out.shape[3]), int(out.shape[4])
    host = torch.as_tensor(plan, dtype=torch.int32).reshape(-1).contiguous()
    dev = host.to(actor.device, non_blocking=False)
    counts = torch.empty(int(nclips), dtype=torch.int32, device=actor.device)
    m3, inv3 = _mean_inv_std(mean, std)
    check(lib().bdv_actor_cut_mix_u8(_p(actor), n_actor, Ha, Wa, _p(scene), n_scene, Hs, Ws, _p(dev), host.data_ptr(), int(host.numel()),
                                     int(nclips), T, Hd, Wd, m3, inv3, _p(out), B_out, _p(counts), _stream()), 'bdv_actor_cut_mix_u8')
    return counts


def gradcam_map(act, wgt):
    """``bdv_gradcam_map``: act (N, h, w, C) fp32 NHWC, wgt (N, C) fp32 -> (N, h, w) = relu(sum_c wgt[n, c] * act[n, y, x, c])."""
    _chk(act, name='act')
    if act.dim() != 4:
        raise ValueError(f'gradcam_map: act must be (N, h, w, C), got {tuple(act.shape)}')
    N, h, w, C = (int(d) for d in act.shape)
    if N == 0 or h * w == 0 or C == 0 or C % 4:
        raise ValueError(f'gradcam_map: act {tuple(act.shape)}: every dimension must be positive and C a multiple of 4')
    _chk(wgt, (N, C), name='wgt')
    out = torch.empty((N, h, w), dtype=torch.float32, device=act.device)
    check(lib().bdv_gradcam_map(_p(act), _p(wgt), _p(out), N, h * w, C, _stream()), 'bdv_gradcam_map')
    return out


def _gradcam_dims(m, B, T, H, W, who):
    _chk(m, name='map')
    B, T, H, W = int(B), int(T), int(H), int(W)
    if m.dim() != 3 or B <= 0 or T <= 0 or m.shape[0] != B * T or m.shape[1] == 0 or m.shape[2] == 0:
        raise ValueError(f'{who}: map must be (B*T, h, w) = ({B * T}, h, w), got {tuple(m.shape)}')
    if H <= 0 or W <= 0:
        raise ValueError(f'{who}: output size {(H, W)} must be positive')
    return B, T, int(m.shape[1]), int(m.shape[2]), H, W


def gradcam_minmax(m, B: int, T: int, H: int, W: int):
    """``bdv_gradcam_minmax``: m (B*T, h, w) fp32, non-negative -> (2, B): per clip the minimum (row 0) and maximum (row 1) of the map
    upsampled per frame to (H, W) (bilinear, align_corners=False)."""
    B, T, h, w, H, W = _gradcam_dims(m, B, T, H, W, 'gradcam_minmax')
    out = torch.empty((2, B), dtype=torch.float32, device=m.device)
    check(lib().bdv_gradcam_minmax(_p(m), B, T, h, w, H, W, _p(out), _stream()), 'bdv_gradcam_minmax')
    return out


def gradcam_render(m, minmax, B: int, T: int, H: int, W: int, want_map: bool = True, frames4=None, lut=None, alpha: float = 0.5,
                   mean=None, std=None, box_offsets=None, boxes=None):
    """``bdv_gradcam_render``: m (B*T, h, w), minmax (2, B) from ``gradcam_minmax`` -> ``(v, overlay, sums)``, each None unless asked for:
    v (B, T, H, W) fp32 when ``want_map``; overlay (B, T, H, W, 3) uint8 when ``frames4`` (B*T, H, W, 4) -- the normalised frames --
    is given, with ``lut`` (256, 3) fp32 on the device, ``alpha``, and the Normalize ``mean`` / ``std``; sums (B, 2) fp32 =
    (sum v, sum v inside the boxes) when ``box_offsets`` (B*T + 1,) and ``boxes`` (n, 4) -- host arrays, x0 y0 x1 y1 in output
    pixels -- are given.  The tables are validated on the host (here and in the library) before the launch."""
    B, T, h, w, H, W = _gradcam_dims(m, B, T, H, W, 'gradcam_render')
    _chk(minmax, (2, B), name='minmax')
    dev = m.device
    v = torch.empty((B, T, H, W), dtype=torch.float32, device=dev) if want_map else None
    overlay, f3 = None, ctypes.c_float * 3
    mean3, std3 = f3(0.0, 0.0, 0.0), f3(1.0, 1.0, 1.0)
    if frames4 is not None:
        _chk(frames4, (B * T, H, W, 4), name='frames4')
        if lut is None or mean is None or std is None:
            raise ValueError('gradcam_render: the overlay needs lut, mean and std')
        _chk(lut, (256, 3), name='lut')
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f'gradcam_render: alpha {alpha} outside [0, 1]')
        mean3 = f3(*torch.tensor(list(mean), dtype=torch.float32).tolist())
        std3 = f3(*torch.tensor(list(std), dtype=torch.float32).tolist())
        overlay = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device=dev)
    sums = off_h = box_h = off_d = box_d = ws = None
    nbox, ws_bytes = 0, 0
    if (box_offsets is None) != (boxes is None):
        raise ValueError('gradcam_render: box_offsets and boxes come together')
    if box_offsets is not None:
        off64 = torch.as_tensor(box_offsets).to('cpu').reshape(-1)
        if off64.is_floating_point() or off64.dtype == torch.bool:
            raise TypeError(f'gradcam_render: box_offsets must be integers, got {off64.dtype}')
        off64 = off64.to(torch.int64)
        box_h = torch.as_tensor(boxes).to('cpu', torch.float32).contiguous()
        if box_h.numel() == 0:
            box_h = box_h.reshape(0, 4)
        if box_h.dim() != 2 or box_h.shape[1] != 4:
            raise ValueError(f'gradcam_render: boxes must be (n, 4), got {tuple(box_h.shape)}')
        nbox = int(box_h.shape[0])
        if off64.numel() != B * T + 1:
            raise ValueError(f'gradcam_render: {off64.numel()} box offsets for {B * T} frames ({B * T + 1} expected)')
        if int(off64[0]) != 0 or bool((off64[1:] < off64[:-1]).any()):
            raise ValueError('gradcam_render: box offsets must start at 0 and must not decrease')
        if int(off64[-1]) != nbox:
            raise ValueError(f'gradcam_render: the box offsets end at {int(off64[-1])}, the table has {nbox} rows')
        if bool(torch.isnan(box_h).any()):
            raise ValueError('gradcam_render: a box holds a NaN')
        off_h = off64.to(torch.int32).contiguous()
        off_d, box_d = off_h.to(dev), (box_h.to(dev) if nbox else None)
        sums = torch.empty((B, 2), dtype=torch.float32, device=dev)
        ws_bytes = int(lib().bdv_gradcam_workspace_bytes(B, T, H))
        ws = workspace(ws_bytes, dev, 'gradcam')
    if v is None and overlay is None and sums is None:
        raise ValueError('gradcam_render: nothing requested (want_map, frames4 or boxes)')
    check(lib().bdv_gradcam_render(_p(m), _p(minmax), B, T, h, w, H, W, _p(v), _p(frames4), _p(lut), float(alpha), mean3, std3, _p(overlay),
                                   _p(off_d), off_h.data_ptr() if off_h is not None else None, _p(box_d),
                                   box_h.data_ptr() if nbox else None, nbox, _p(sums), _p(ws), ws_bytes, _stream()), 'bdv_gradcam_render')
    return v, overlay, sums

WGRAD_X3 = _x3_default('BDVCIL_WGRAD_X3')


def conv_wgrad_partial(dy: torch.Tensor, x: torch.Tensor, g: ConvGeom, x3: Optional[bool] = None,
                       dw: Optional[torch.Tensor] = None, pre_bn=None):
    """Split-K partial products of a weight gradient -> (slab (splits, Cout, R, S, Cin), empty dw); reduce them later with
    ``wgrad_reduce_batched`` (the slab must stay alive until then)."""
    g.act_dtype = _act_code(dy)
    _chk_conv(dy, (g.N, g.Ho, g.Wo, g.Cout), g, 'dy')
    _chk_conv(x, (_in_frames(g), g.H, g.W, g.Cin), g, 'x')
    use_x3 = WGRAD_X3 if x3 is None else x3
    _chk_bf16_arith(g, use_x3, 'conv_wgrad_partial')
    plan = conv_plan(g, 'wgrad', use_x3, pre_bn is not None)
    if pre_bn is not None:      # x = the producer's raw conv output; its BatchNorm + ReLU is applied in the loader
        _chk(pre_bn[0], (g.Cin,), name='pre_scale')
        _chk(pre_bn[1], (g.Cin,), name='pre_shift')
    slab = torch.empty((plan.splits, g.Cout, _taps_r(g), g.S, g.Cin), dtype=torch.float32, device=dy.device)
    if use_x3 and PIECES == F16X2:
        f16 = _plan_f16(plan)
        check(lib().bdv_conv_wgrad_partial_f16x2(_p(dy), _p(act_amax(dy) if f16 else None), _p(x), _p(act_amax(x) if f16 else None),
                                                 ctypes.byref(g), _p(slab), slab.numel() * 4,
                                                 _p(pre_bn[0] if pre_bn is not None else None), _p(pre_bn[1] if pre_bn is not None else None),
                                                 _stream()), 'bdv_conv_wgrad_partial_f16x2')
    elif use_x3:
        check(lib().bdv_conv_wgrad_partial_pl(_p(dy), _p(x), ctypes.byref(g), _p(slab), slab.numel() * 4, PIECES,
                                              _p(pre_bn[0] if pre_bn is not None else None), _p(pre_bn[1] if pre_bn is not None else None),
                                              _stream()), 'bdv_conv_wgrad_partial_pl')
    else:
        check(lib().bdv_conv_wgrad_partial(_p(dy), _p(x), ctypes.byref(g), _p(slab), slab.numel() * 4, _stream()), 'bdv_conv_wgrad_partial')
    if dw is None:
        dw = torch.empty((g.Cout, _taps_r(g), g.S, g.Cin), dtype=torch.float32, device=dy.device)
    return slab, dw


def wgrad_reduce_batched(items, beta: float = 0.0):
    """items: [(slab, dw), ...] from ``conv_wgrad_partial``; dw[k] = beta * dw[k] + sum over the slices of slab[k], for all
    items in as few launches as BDV_MAX_REDUCE_ITEMS allows."""
    MAXN = 32
    for a in range(0, len(items), MAXN):
        chunk = items[a:a + MAXN]
        n = len(chunk)
        for slab, dw in chunk:
            _chk(slab, name='slab')
            _chk(dw, name='dw')
            if slab.shape[1:] != dw.shape:
                raise ValueError(f'wgrad_reduce_batched: slab {tuple(slab.shape)} does not stack dw {tuple(dw.shape)}')
        slabs = (ctypes.c_void_p * n)(*[s.data_ptr() for s, _ in chunk])
        dws = (ctypes.c_void_p * n)(*[d.data_ptr() for _, d in chunk])
        splits = (ctypes.c_int * n)(*[s.shape[0] for s, _ in chunk])
        numels = (ctypes.c_int64 * n)(*[d.numel() for _, d in chunk])
        check(lib().bdv_wgrad_reduce_batched(ctypes.cast(slabs, ctypes.c_void_p), ctypes.cast(dws, ctypes.c_void_p),
                                             ctypes.cast(splits, ctypes.c_void_p), ctypes.cast(numels, ctypes.c_void_p), n,
                                             float(beta), _stream()), 'bdv_wgrad_reduce_batched')


# ---------------------------------------------------------------------------------------------
# heads / losses
# ---------------------------------------------------------------------------------------------

def lsc_fwd(x, w, K, P):
    _chk(x, name='x')
    N, D = x.shape
    _chk(w, (K, P * D), name='w')
    sim = torch.empty((N, K), dtype=torch.float32, device=x.device)
    xnorm = torch.empty(N, dtype=torch.float32, device=x.device)
    wnorm = torch.empty(K * P, dtype=torch.float32, device=x.device)
    cosbuf = torch.empty((N, K * P), dtype=torch.float32, device=x.device)
    check(lib().bdv_lsc_fwd(_p(x), _p(w), _p(sim), _p(xnorm), _p(wnorm), _p(cosbuf), N, D, K, P, _stream()), 'bdv_lsc_fwd')
    return sim, xnorm, wnorm, cosbuf


def lsc_bwd(dsim, x, w, xnorm, wnorm, cosbuf, K, P, need_dw=True, dw=None, beta_w=0.0):
    N, D = x.shape
    _chk(dsim, (N, K), name='dsim')
    _chk(x, name='x')
    _chk(w, (K, P * D), name='w')
    _chk(xnorm, (N,), name='xnorm')
    _chk(wnorm, (K * P,), name='wnorm')
    _chk(cosbuf, (N, K * P), name='cosbuf')
    dx = torch.empty_like(x)
    if need_dw and dw is None:
        dw = torch.empty_like(w)
        beta_w = 0.0
    if dw is not None:
        _chk(dw, (K, P * D), name='dw')
    ws = torch.empty((N, K * P), dtype=torch.float32, device=x.device)
    check(lib().bdv_lsc_bwd(_p(dsim), _p(x), _p(w), _p(xnorm), _p(wnorm), _p(cosbuf), _p(dx), _p(dw if need_dw else None),
                            float(beta_w), _p(ws), N, D, K, P, _stream()), 'bdv_lsc_bwd')
    return dx, (dw if need_dw else None)


def linear_fwd(x, w, b):
    _chk(x, name='x')
    N, D = x.shape
    K = w.shape[0]
    _chk(w, (K, D), name='w')
    if b is not None:
        _chk(b, (K,), name='b')
    out = torch.empty((N, K), dtype=torch.float32, device=x.device)
    check(lib().bdv_linear_fwd(_p(x), _p(w), _p(b), _p(out), N, D, K, _stream()), 'bdv_linear_fwd')
    return out


def linear_bwd(dout, x, w, need_dx=True, need_dw=True, need_db=True, dw=None, db=None, beta_w=0.0):
    N, D = x.shape
    K = w.shape[0]
    _chk(dout, (N, K), name='dout')
    _chk(x, name='x')
    _chk(w, (K, D), name='w')
    dx = torch.empty_like(x) if need_dx else None
    if need_dw and dw is None:
        dw = torch.empty_like(w)
        db = torch.empty(K, dtype=torch.float32, device=x.device) if need_db else None
        beta_w = 0.0
    if need_dw:
        _chk(dw, (K, D), name='dw')
        if db is not None:
            _chk(db, (K,), name='db')
    check(lib().bdv_linear_bwd(_p(dout), _p(x), _p(w), _p(dx), _p(dw if need_dw else None), _p(db if need_dw else None),
                               float(beta_w), N, D, K, _stream()), 'bdv_linear_bwd')
    return dx, (dw if need_dw else None), (db if need_dw else None)


def consensus_fwd(s, B, T):
    _chk(s, name='s')
    K = s.shape[1]
    if s.shape[0] != B * T:
        raise ValueError(f'consensus_fwd: {s.shape[0]} rows != B*T = {B * T}')
    out = torch.empty((B, K), dtype=torch.float32, device=s.device)
    check(lib().bdv_consensus_fwd(_p(s), _p(out), B, T, K, _stream()), 'bdv_consensus_fwd')
    return out


def consensus_bwd(dout, T):
    _chk(dout, name='dout')
    B, K = dout.shape
    ds = torch.empty((B * T, K), dtype=torch.float32, device=dout.device)
    check(lib().bdv_consensus_bwd(_p(dout), _p(ds), B, T, K, _stream()), 'bdv_consensus_bwd')
    return ds


def dropout(x, p, seed):
    _chk(x, name='x')
    out = torch.empty_like(x)
    check(lib().bdv_dropout(_p(x), _p(out), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), 'bdv_dropout')
    return out


def lsc_loss(sim, targets, eta, margin, hinge, class_weights=None):
    _chk(sim, name='sim')
    B, K = sim.shape
    _chk(targets, (B,), dtype=torch.int64, name='targets')
    _chk(eta, (1,), name='eta')
    if class_weights is not None:
        _chk(class_weights, (K,), name='class_weights')
    out = torch.empty(2, dtype=torch.float32, device=sim.device)   # loss, deta
    dsim = torch.empty_like(sim)
    check(lib().bdv_lsc_loss(_p(sim), _p(targets), _p(eta), float(margin), int(bool(hinge)), _p(class_weights), _p(out[0:1]),
                             _p(dsim), _p(out[1:2]), B, K, _stream()), 'bdv_lsc_loss')
    return out[0], dsim, out[1:2]


def softce_loss(score, soft_targets=None, labels=None):
    _chk(score, name='score')
    B, K = score.shape
    if soft_targets is not None:
        _chk(soft_targets, (B, K), name='soft_targets')
    else:
        _chk(labels, (B,), dtype=torch.int64, name='labels')
    loss = torch.empty(1, dtype=torch.float32, device=score.device)
    dscore = torch.empty_like(score)
    check(lib().bdv_softce_loss(_p(score), _p(soft_targets), _p(labels), _p(loss), _p(dscore), B, K, _stream()),
          'bdv_softce_loss')
    return loss[0], dscore


def icarl_targets(labels, prev_logits, prev_K, K, base_targets=None):
    """(B, K) targets of ICARLModel.training_step: ``base_targets`` (or one-hot), old-class rows <- softmax(prev logits)."""
    B = labels.numel()
    labels = labels.reshape(B)
    _chk(labels, (B,), dtype=torch.int64, name='labels')
    if prev_logits is not None:
        _chk(prev_logits, (B, K), name='prev_logits')
    if base_targets is not None:
        _chk(base_targets, (B, K), name='base_targets')
    tgt = torch.empty((B, K), dtype=torch.float32, device=labels.device)
    check(lib().bdv_icarl_targets(_p(labels), _p(prev_logits), int(prev_K), _p(base_targets), _p(tgt), B, K, _stream()),
          'bdv_icarl_targets')
    return tgt


def acm_targets(labels, background_labels, foreground_ratio, alpha, K):
    """ACMSmoothCE smooth labels (libs/losses/acm_smooth_ce.py:18-28) -> (B, K)."""
    B = labels.numel()
    labels = labels.reshape(B)
    _chk(labels, (B,), dtype=torch.int64, name='labels')
    _chk(background_labels, (B,), dtype=torch.int64, name='background_labels')
    _chk(foreground_ratio, (B,), name='foreground_ratio')
    tgt = torch.empty((B, K), dtype=torch.float32, device=labels.device)
    check(lib().bdv_acm_targets(_p(labels), _p(background_labels), _p(foreground_ratio), float(alpha), _p(tgt), B, K, _stream()),
          'bdv_acm_targets')
    return tgt


def softmax_mean(s, B, n, apply_softmax=True):
    _chk(s, name='s')
    K = s.shape[1]
    if s.shape[0] != B * n:
        raise ValueError('softmax_mean: row count mismatch')
    out = torch.empty((B, K), dtype=torch.float32, device=s.device)
    check(lib().bdv_softmax_mean(_p(s), _p(out), B, n, K, int(bool(apply_softmax)), _stream()), 'bdv_softmax_mean')
    return out


def topk_acc(score, labels):
    _chk(score, name='score')
    B, K = score.shape
    _chk(labels, (B,), dtype=torch.int64, name='labels')
    acc = torch.empty(2, dtype=torch.float32, device=score.device)
    check(lib().bdv_topk_acc(_p(score), _p(labels), _p(acc), B, K, _stream()), 'bdv_topk_acc')
    return acc


def kd_mse_fwd(cur, prev):
    """cur/prev: any same-shape, same-stride dense tensors (compared in storage order)."""
    if cur.shape != prev.shape or cur.stride() != prev.stride() or cur.dtype != prev.dtype:
        raise ValueError('kd_mse: cur and prev need identical shape, strides and dtype')
    a, b = _dense_storage(cur), _dense_storage(prev)
    mse = torch.empty(1, dtype=torch.float32, device=cur.device)
    ws = workspace(lib().bdv_reduce_workspace_bytes(), cur.device, 'red')
    check(lib().bdv_kd_mse_fwd(_p(a), _p(b), _p(mse), a.numel(), _p(ws), ws.numel(), _act_code(a), _stream()), 'bdv_kd_mse_fwd')
    return mse[0]


def kd_mse_bwd(cur, prev, gscale_dev, gscale_host=1.0):
    a, b = _dense_storage(cur), _dense_storage(prev)
    d = torch.empty_like(cur)        # preserves strides for dense tensors
    if d.stride() != cur.stride():
        raise ValueError('kd_mse_bwd: could not preserve strides')
    if gscale_dev is not None:
        _gscale(gscale_dev, 'gscale')
    check(lib().bdv_kd_mse_bwd(_p(a), _p(b), _p(gscale_dev), float(gscale_host), _p(_dense_storage(d)), a.numel(), _act_code(a), _stream()),
          'bdv_kd_mse_bwd')
    return d


def _kd_nhwc(t: torch.Tensor, name: str, dtypes=(torch.float32, torch.bfloat16), allow_2d: bool = False) -> torch.Tensor:
    """The (N, H, W, C) storage of a hooked KD module's output, logically (N, C, H, W) -- with ``allow_2d`` also (N, D), taken as
    (N, D, 1, 1): channels-last strides are used in place, any other layout costs one copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a tensor, got {type(t)}')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: the HIP path needs a GPU tensor (got device {t.device}); there is no CPU fallback')
    if t.dtype not in dtypes:
        raise TypeError(f'{name}: dtype {t.dtype}, expected {" or ".join(map(str, dtypes))}')
    if allow_2d and t.dim() == 2:
        t = t[:, :, None, None]
    if t.dim() != 4:
        raise ValueError(f'{name}: expected ' + ('(N, C, H, W), (N, D, 1, 1) or (N, D)' if allow_2d else 'a 4-D (N, C, H, W) tensor')
                         + f', got shape {tuple(t.shape)}')
    p = t.permute(0, 2, 3, 1)
    return p if p.is_contiguous() else p.contiguous()


def _kd_pair(cur: torch.Tensor, prev: torch.Tensor, who: str):
    if cur.shape != prev.shape or cur.dtype != prev.dtype:
        raise ValueError(f'{who}: cur {tuple(cur.shape)} {cur.dtype} and prev {tuple(prev.shape)} {prev.dtype} differ')


def _gscale(t: torch.Tensor, name: str) -> torch.Tensor:
    """The upstream gradient of a distillation loss: one fp32 value in device memory."""
    return _chk(t.reshape(1), (1,), name=name)


def _with_strides_of(d_nhwc: torch.Tensor, cur: torch.Tensor) -> torch.Tensor:
    """The (N, H, W, C) gradient storage ``d_nhwc`` as a tensor of ``cur``'s logical shape and strides: a view when ``cur`` holds its
    elements in that order (channels-last maps, (N, D, 1, 1) and (N, D) features), one copy otherwise."""
    d = d_nhwc.permute(0, 3, 1, 2).view(cur.shape)
    if all(sd == sc for sd, sc, n in zip(d.stride(), cur.stride(), cur.shape) if n > 1):
        return d.as_strided(cur.shape, cur.stride())     # only the strides of dimensions of length 1 can differ
    out = torch.empty_like(cur)
    out.copy_(d)
    return out


def pod_spatial_fwd(cur, prev):
    """POD-spatial distillation loss (csrc/pod_kd.hip) of logical (N, C, H, W) maps.  Returns ``(loss, G, cur_nhwc)``: the scalar,
    the profile gradient (N, H+W, C) fp32 and the (N, H, W, C) storage of ``cur`` that was read (``cur``'s own when it is
    channels-last), which together are what ``pod_spatial_bwd`` needs."""
    a, b = _kd_nhwc(cur, 'pod_spatial: cur'), _kd_nhwc(prev, 'pod_spatial: prev')
    _kd_pair(cur, prev, 'pod_spatial')
    N, H, W, C = a.shape
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    G = torch.empty((N, H + W, C), dtype=torch.float32, device=a.device)
    ws = workspace(lib().bdv_pod_workspace_bytes(N, C, H, W), a.device, 'pod')
    check(lib().bdv_pod_spatial_fwd(_p(a), _p(b), _p(loss), _p(G), N, C, H, W, _p(ws), ws.numel(), _act_code(a), _stream()),
          'bdv_pod_spatial_fwd')
    return loss[0], G, a


def pod_spatial_bwd(cur, G, gscale_dev):
    """``dcur = gscale * 2 * cur * (G[n,h,c] + G[n,H+w,c])`` for the logical (N, C, H, W) ``cur``, in ``cur``'s strides and dtype."""
    a = _kd_nhwc(cur, 'pod_spatial_bwd: cur')
    N, H, W, C = a.shape
    _chk(G, (N, H + W, C), name='pod_spatial_bwd: G')
    _gscale(gscale_dev, 'pod_spatial_bwd: gscale')
    d = torch.empty_like(a)
    check(lib().bdv_pod_spatial_bwd(_p(a), _p(G), _p(gscale_dev), _p(d), N, C, H, W, _act_code(a), _stream()), 'bdv_pod_spatial_bwd')
    return _with_strides_of(d, cur)


def pod_flat(cur, prev):
    """POD-flat (cosine embedding) distillation loss of (N, D) or (N, D, 1, 1) features.  Returns ``(loss, dcur_unit)`` with
    ``dcur_unit`` (N, D) fp32 the gradient for an upstream gradient of 1."""
    a, b = _kd_nhwc(cur, 'pod_flat: cur', allow_2d=True), _kd_nhwc(prev, 'pod_flat: prev', allow_2d=True)
    _kd_pair(cur, prev, 'pod_flat')
    N, H, W, D = a.shape
    if H * W != 1:
        raise ValueError(f'pod_flat: expected (N, D) or (N, D, 1, 1) features, got shape {tuple(cur.shape)}')
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    d = torch.empty((N, D), dtype=torch.float32, device=a.device)
    ws = workspace(lib().bdv_pod_workspace_bytes(N, D, 1, 1), a.device, 'pod')
    check(lib().bdv_pod_flat(_p(a), _p(b), _p(loss), _p(d), N, D, _p(ws), ws.numel(), _act_code(a), _stream()), 'bdv_pod_flat')
    return loss[0], d


def _tc_map(table: torch.Tensor, N: int, C: int, name: str, what: str = 'importance') -> torch.Tensor:
    """The fp32 (T, C) table of the time-channel kernels -- the importance map or the accumulator -- for N frames of C channels."""
    _chk(table, name=f'{name}: {what}')
    if table.dim() != 2 or table.shape[1] != C or table.shape[0] == 0 or N % table.shape[0] != 0:
        raise ValueError(f'{name}: {what} of shape {tuple(table.shape)} for {N} frames of {C} channels; expected (T, C) with '
                         f'T dividing the frame count')
    return table


def kd_tc_fwd(cur, prev, importance):
    """Time-channel weighted distillation loss (csrc/tc_kd.hip): mean over all elements of ``importance[n mod T, c] * (cur - prev)^2``
    for hooked outputs of shape (N, C, H, W), (N, D, 1, 1) or (N, D) and an fp32 (T, C) map."""
    a, b = _kd_nhwc(cur, 'kd_tc: cur', allow_2d=True), _kd_nhwc(prev, 'kd_tc: prev', allow_2d=True)
    _kd_pair(cur, prev, 'kd_tc')
    N, H, W, C = a.shape
    A = _tc_map(importance, N, C, 'kd_tc')
    T = A.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = workspace(lib().bdv_kd_tc_workspace_bytes(N, T, C, H, W), a.device, 'tc')
    check(lib().bdv_kd_tc_fwd(_p(a), _p(b), _p(A), _p(loss), N, T, C, H, W, _p(ws), ws.numel(), _act_code(a), _stream()), 'bdv_kd_tc_fwd')
    return loss[0]


def kd_tc_bwd(cur, prev, importance, gscale_dev):
    """``dcur = gscale * 2 / numel * importance[n mod T, c] * (cur - prev)`` in ``cur``'s shape, strides and dtype."""
    a, b = _kd_nhwc(cur, 'kd_tc_bwd: cur', allow_2d=True), _kd_nhwc(prev, 'kd_tc_bwd: prev', allow_2d=True)
    _kd_pair(cur, prev, 'kd_tc_bwd')
    N, H, W, C = a.shape
    A = _tc_map(importance, N, C, 'kd_tc_bwd')
    _gscale(gscale_dev, 'kd_tc_bwd: gscale')
    # a is cur's own storage when cur is channels-last: a gradient allocated like it is then written in place, with no copy after
    d = torch.empty_like(a)
    check(lib().bdv_kd_tc_bwd(_p(a), _p(b), _p(A), _p(gscale_dev), _p(d), N, A.shape[0], C, H, W, _act_code(a), _stream()), 'bdv_kd_tc_bwd')
    return _with_strides_of(d, cur)


def tc_sqgrad_accum(S, grad, scale):
    """``S[t, c] += scale^2 * sum_{b,h,w} grad[b*T+t, c, h, w]^2`` in place, for an fp32 gradient at a hooked module and the fp32
    (T, C) accumulator ``S`` (csrc/tc_kd.hip): two stages in a fixed order, so ``S`` is bitwise reproducible."""
    g = _kd_nhwc(grad, 'tc_sqgrad_accum: grad', dtypes=(torch.float32,), allow_2d=True)
    N, H, W, C = g.shape
    _tc_map(S, N, C, 'tc_sqgrad_accum', 'S')
    T = S.shape[0]
    ws = workspace(lib().bdv_kd_tc_workspace_bytes(N, T, C, H, W), g.device, 'tc')
    check(lib().bdv_tc_sqgrad_accum(_p(g), _p(S), float(scale), N, T, C, H, W, _p(ws), ws.numel(), _stream()), 'bdv_tc_sqgrad_accum')
    return S


def _dense_storage(t: torch.Tensor) -> torch.Tensor:
    """Flat view over the storage of a dense (possibly permuted) tensor."""
    if not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError('expected an fp32 (or, in the bf16-storage mode, bf16) GPU tensor; there is no CPU fallback')
    if t.is_contiguous():
        return t.reshape(-1)
    order = sorted(range(t.dim()), key=lambda i: -t.stride(i))
    p = t.permute(order)
    if not p.is_contiguous():
        raise ValueError('tensor is not dense')
    return p.reshape(-1)


# ---------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------

def multi_sqnorm(grad_ptrs, numels, ntensors, out):
    ws = workspace(ntensors * 32 * 4, out.device, 'sqn')
    check(lib().bdv_multi_sqnorm(_p(grad_ptrs), _p(numels), ntensors, _p(out), _p(ws), ws.numel(), _stream()), 'bdv_multi_sqnorm')


def clip_coef(sqnorm, grad_scale, max_norm, coef):
    check(lib().bdv_clip_coef(_p(sqnorm), float(grad_scale), float(max_norm), _p(coef), _stream()), 'bdv_clip_coef')


def multi_sgd(param_ptrs, grad_ptrs, buf_ptrs, numels, lrs, wds, ntensors, momentum, grad_scale, coef):
    check(lib().bdv_multi_sgd(_p(param_ptrs), _p(grad_ptrs), _p(buf_ptrs), _p(numels), _p(lrs), _p(wds), ntensors,
                              float(momentum), float(grad_scale), _p(coef), _stream()), 'bdv_multi_sgd')


# ---------------------------------------------------------------------------------------------
# representation path (clip representations, NME classifier, class means, herding)
# ---------------------------------------------------------------------------------------------

def repr_from_features(feat, B, crops, T):
    """feat (B*crops*T, D) -> (repr (B, crops, D), mean_crops (B, D)); libs/cil/cil.py:501-506,:564-571."""
    _chk(feat, name='feat')
    if feat.dim() != 2 or feat.shape[0] != B * crops * T:
        raise ValueError(f'repr_from_features: feat {tuple(feat.shape)} is not (B*crops*T = {B * crops * T}, D)')
    D = feat.shape[1]
    rp = torch.empty((B, crops, D), dtype=torch.float32, device=feat.device)
    mc = torch.empty((B, D), dtype=torch.float32, device=feat.device)
    check(lib().bdv_repr_from_features(_p(feat), _p(rp), _p(mc), B, crops, T, D, _stream()), 'bdv_repr_from_features')
    return rp, mc


def nme_classify(repr_, class_means):
    """repr_ (S, crops, D), class_means (K, D) -> (similarity (S, K), pred (S,) int64); libs/cil/cil.py:945-960."""
    _chk(repr_, name='repr_')
    _chk(class_means, name='class_means')
    if repr_.dim() != 3 or class_means.dim() != 2 or repr_.shape[2] != class_means.shape[1]:
        raise ValueError(f'nme_classify: repr_ {tuple(repr_.shape)} vs class_means {tuple(class_means.shape)}')
    S, crops, D = repr_.shape
    Kc = class_means.shape[0]
    sim = torch.empty((S, Kc), dtype=torch.float32, device=repr_.device)
    pred = torch.empty((S,), dtype=torch.int64, device=repr_.device)
    ws = workspace(lib().bdv_nme_workspace_bytes(Kc, D), repr_.device, 'nme')
    check(lib().bdv_nme_classify(_p(repr_), _p(class_means), _p(sim), _p(pred), S, crops, D, Kc, _p(ws), ws.numel(), _stream()),
          'bdv_nme_classify')
    return sim, pred


def class_means(repr_, labels, num_classes):
    """repr_ (n, D), labels (n,) int64 -> (num_classes, D) per-class means; libs/cil/cil.py:1079-1083."""
    _chk(repr_, name='repr_')
    _chk(labels, (repr_.shape[0],), dtype=torch.int64, name='labels')
    n, D = repr_.shape
    out = torch.empty((num_classes, D), dtype=torch.float32, device=repr_.device)
    check(lib().bdv_class_means(_p(repr_), _p(labels), _p(out), n, D, int(num_classes), _stream()), 'bdv_class_means')
    return out


def herding_select(features, num_exemplars, cosine_distance):
    """features (n, D) of one class -> (class_mean (1, D), indices (m,) int64, dist (m,)); memory_selection.py:70-92."""
    _chk(features, name='features')
    if features.dim() != 2:
        raise ValueError(f'herding_select: features must be (n, D), got {tuple(features.shape)}')
    n, D = features.shape
    m = int(num_exemplars)
    cm = torch.empty((1, D), dtype=torch.float32, device=features.device)
    idx = torch.empty((max(m, 1),), dtype=torch.int64, device=features.device)
    dist = torch.empty((max(m, 1),), dtype=torch.float32, device=features.device)
    ws = workspace(lib().bdv_herding_workspace_bytes(n, D), features.device, 'herding')
    check(lib().bdv_herding_select(_p(features), n, D, m, int(bool(cosine_distance)), _p(cm), _p(idx), _p(dist), _p(ws),
                                   ws.numel(), _stream()), 'bdv_herding_select')
    return cm, idx[:m], dist[:m]


# ---- data path: RandAugment on uint8 frames ---------------------------------------------------------------------------

RANDAUG_NUM_OPS = 12


def randaug_apply(frames_u8, op_i, op_d, out=None):
    """One operation slot of RandAugment for a batch of clips.  frames_u8 (B, T, H, W, 3) uint8; op_i (B, 8) int32 and
    op_d (B, 4) float64 device tables (layout: include/bdvcil_hip.h, bdv_randaug_apply) -> new (B, T, H, W, 3) uint8."""
    _chk(frames_u8, dtype=torch.uint8, name='frames_u8')
    if frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
        raise ValueError(f'randaug_apply: frames must be (B, T, H, W, 3), got {tuple(frames_u8.shape)}')
    B, T, H, W, _ = frames_u8.shape
    _chk(op_i, (B, 8), torch.int32, 'op_i')
    _chk(op_d, (B, 4), torch.float64, 'op_d')
    if out is None:
        out = torch.empty_like(frames_u8)
    else:
        _chk(out, frames_u8.shape, torch.uint8, 'out')
        if out.data_ptr() == frames_u8.data_ptr():
            raise ValueError('randaug_apply: out must not alias the input')
    ws = workspace(lib().bdv_randaug_workspace_bytes(B, T, H, W), frames_u8.device, 'randaug')
    check(lib().bdv_randaug_apply(_p(frames_u8), _p(out), _p(op_i), _p(op_d), B, T, H, W, _p(ws), ws.numel(), _stream()),
          'bdv_randaug_apply')
    return out


# ---- clip blending: train_cfg.blending (Mixup / CutMix) and VideoMix -----------------------------------------------------------

def _blend_perm(perm, B: int, device, who: str) -> torch.Tensor:
    """The HOST index vector of a blend (``torch.randperm`` output, a list) -> device int64 (B,).  Its range is checked here, on the
    host copy, so the kernels never form an address outside the batch and nothing is copied back."""
    if isinstance(perm, torch.Tensor) and perm.is_cuda:
        raise TypeError(f'{who}: perm must be a host tensor (its range is checked before the upload)')
    host = torch.as_tensor(perm, dtype=torch.int64).reshape(-1).contiguous()
    if host.numel() != B:
        raise ValueError(f'{who}: perm has {host.numel()} entries for a batch of {B}')
    if B and (int(host.min()) < 0 or int(host.max()) >= B):
        raise ValueError(f'{who}: perm entries must lie in [0, {B}), got [{int(host.min())}, {int(host.max())}]')
    return host.to(device)


def blend_mix(x, perm, lam, out=None, perm_dev=None):
    """``bdv_blend_mix_f32``: ``lam * x + (1 - lam) * x[perm]`` over the first dimension of ``x`` (any contiguous fp32 layout), bit for
    bit, as a NEW tensor (or into ``out``, which must not overlap ``x``).  ``perm``: host int64 (B,); ``lam``: a Python float or a
    0-dim host tensor, taken as fp32.  ``perm_dev``: the upload of ``perm`` made by an earlier call's ``_blend_perm``."""
    _chk(x, name='x')
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f'blend_mix: expected a non-empty (B, ...) tensor, got {tuple(x.shape)}')
    B = int(x.shape[0])
    dev = _blend_perm(perm, B, x.device, 'blend_mix') if perm_dev is None else _chk(perm_dev, (B,), torch.int64, 'perm_dev')
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, tuple(x.shape), name='out')
    lam32 = float(torch.as_tensor(lam, dtype=torch.float32))
    check(lib().bdv_blend_mix_f32(_p(x), _p(dev), lam32, _p(out), B, x.numel() // B, _stream()), 'bdv_blend_mix_f32')
    return out


def blend_box_(x, perm, box, outer: int, H: int, W: int, inner: int = 1, perm_dev=None):
    """``bdv_blend_box_f32``, in place: ``x[b, :, r1:r2, c1:c2, :] = x[perm[b], :, r1:r2, c1:c2, :]`` (gather, then assign) on samples of
    ``outer * H * W * inner`` floats; ``box = (r1, c1, r2, c2)``.  The batch size is ``x.numel()`` over the sample size (the NHWC4
    frames tensor has B * T rows).  Returns ``x``."""
    _chk(x, name='x')
    outer, H, W, inner = int(outer), int(H), int(W), int(inner)
    if inner not in (1, 4) or outer <= 0 or H <= 0 or W <= 0:
        raise ValueError(f'blend_box_: outer {outer}, H {H}, W {W}, inner {inner} (inner is 1 or 4)')
    S = outer * H * W * inner
    if x.numel() == 0 or x.numel() % S:
        raise ValueError(f'blend_box_: {tuple(x.shape)} is not a batch of samples of {outer} x {H} x {W} x {inner}')
    B = x.numel() // S
    r1, c1, r2, c2 = (int(v) for v in box)
    if not (0 <= r1 <= r2 <= H and 0 <= c1 <= c2 <= W):
        raise ValueError(f'blend_box_: box rows {r1}:{r2}, columns {c1}:{c2} outside the {H} x {W} grid')
    dev = _blend_perm(perm, B, x.device, 'blend_box_') if perm_dev is None else _chk(perm_dev, (B,), torch.int64, 'perm_dev')
    if r1 == r2 or c1 == c2:
        return x
    ws = workspace(lib().bdv_blend_box_scratch_bytes(B, outer, inner, r1, c1, r2, c2), x.device, 'blend')
    check(lib().bdv_blend_box_f32(_p(x), _p(dev), B, outer, H, W, inner, r1, c1, r2, c2, _p(ws), ws.numel(), _stream()), 'bdv_blend_box_f32')
    return x


# ---- foreground merging (FAME-style; beyond the reference): csrc/fg_merge.hip -------------------------------------------------------

FG_LAYOUTS = {'tchw': 0, 'thwc4': 1, 'cthw': 2}      # BDV_FG_*: (B,T,3,H,W) | NHWC4 frames (B*T,H,W,4) | (B,3,T,H,W)


def fg_blur_taps(H: int, W: int) -> torch.Tensor:
    """The Gaussian of stage 2 as host fp32 taps: ``k = 2 * (int(0.1 * min(H, W)) // 2) + 1`` of them (23 at 224, 1 = the identity under
    a short side of 20), sigma = k / 3, computed and normalised in fp64."""
    k = 2 * (int(0.1 * min(int(H), int(W))) // 2) + 1
    sigma = k / 3
    j = torch.arange(k, dtype=torch.float64) - (k // 2)
    w = torch.exp(-(j * j) / (2 * sigma * sigma))
    return (w / w.sum()).to(torch.float32)


def fg_colour_params(bins: int, mean, std):
    """Stage 4's six floats: ``lo_c = -mean_c / std_c`` (pixel value 0 after normalisation) and ``s_c = bins * std_c / 256`` (bins per
    normalised unit), formed in fp64 and rounded to fp32.  -> (lo fp32 (3,), scale fp32 (3,)), host tensors."""
    bins = fg_check_bins(bins)
    mean = torch.as_tensor(mean, dtype=torch.float64).reshape(-1)
    std = torch.as_tensor(std, dtype=torch.float64).reshape(-1)
    if mean.numel() != 3 or std.numel() != 3 or not bool((std > 0).all()):
        raise ValueError(f'fg_merge: mean and std must be three numbers each, std positive (got {mean.tolist()}, {std.tolist()})')
    return (-mean / std).to(torch.float32), (bins * std / 256).to(torch.float32)


def fg_check_bins(bins) -> int:
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= 16:
        raise ValueError(f'fg_merge: bins must be an integer in 2..16, got {bins!r}')
    return int(bins)


def fg_k_fg(beta, H: int, W: int) -> int:
    """``max(1, int(beta * H * W))`` for beta in (0, 1]."""
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0 < beta <= 1:
        raise ValueError(f'fg_merge: beta must be a number in (0, 1], got {beta!r}')
    return max(1, int(beta * int(H) * int(W)))


def _fg_dims(B, T, H, W, layout, who):
    B, T, H, W = int(B), int(T), int(H), int(W)
    if layout not in FG_LAYOUTS:
        raise ValueError(f'{who}: layout {layout!r}, expected one of {sorted(FG_LAYOUTS)}')
    if B <= 0 or T <= 0 or H <= 0 or W <= 0 or B > 65535 or H * W > 1 << 24 or T * H * W > 1 << 28:
        raise ValueError(f'{who}: B {B}, T {T}, H {H}, W {W} (B <= 65535, H * W <= 2^24, T * H * W <= 2^28)')
    return B, T, H, W, FG_LAYOUTS[layout], (4 if layout == 'thwc4' else 3)


def _fg_clip(x, B, T, H, W, lanes, who):
    if not isinstance(x, torch.Tensor) or x.numel() != B * T * H * W * lanes:
        raise ValueError(f'{who}: x {tuple(getattr(x, "shape", ()))} is not a batch of {B} clips of {T} x {H} x {W} x {lanes} floats')
    return _chk(x, name=f'{who}: x')


def fg_motion_q(x, B, T, H, W, layout='tchw'):
    """Stages 1-3 (``bdv_fg_motion_q``): -> ``(q uint8, g, d)``, each (B, H, W): the quantised map, the blurred map and the raw motion
    map of every clip of ``x`` (contiguous fp32 in ``layout``)."""
    B, T, H, W, code, lanes = _fg_dims(B, T, H, W, layout, 'fg_motion_q')
    if T < 2:
        raise ValueError(f'fg_motion_q: T {T}: a motion map needs two frames')
    _fg_clip(x, B, T, H, W, lanes, 'fg_motion_q')
    taps = fg_blur_taps(H, W)
    dev = x.device
    d, tmp, g = (torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(3))
    mm = torch.empty((B, 2), dtype=torch.int32, device=dev)
    part = workspace(B * ((H * W + 255) // 256) * 8, dev, 'fg_minmax')
    q = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    check(lib().bdv_fg_motion_q(_p(x), B, T, H, W, code, ctypes.c_void_p(taps.data_ptr()), taps.numel(), _p(d), _p(tmp), _p(g), _p(part), _p(mm),
                                _p(q), _stream()), 'bdv_fg_motion_q')
    return q, g, d


def fg_hist_refine(x, q, B, T, H, W, layout='tchw', bins=8, lo=None, scale=None):
    """Stages 4-5 (``bdv_fg_hist_refine``): -> ``(s (B, H, W) fp32, F, N)`` with F, N (B, bins^3) int32 tensors holding the uint32 sums of
    ``q`` and the counts per colour bin.  ``lo`` / ``scale``: host triples of ``fg_colour_params``."""
    B, T, H, W, code, lanes = _fg_dims(B, T, H, W, layout, 'fg_hist_refine')
    bins = fg_check_bins(bins)
    if 255 * T * H * W >= 1 << 32:
        raise ValueError(f'fg_hist_refine: 255 * T * H * W = 255 * {T} * {H} * {W} does not fit the uint32 histograms')
    if not isinstance(q, torch.Tensor) or q.numel() != B * H * W:
        raise ValueError(f'fg_hist_refine: q {tuple(getattr(q, "shape", ()))} is not ({B}, {H}, {W})')
    _fg_clip(x, B, T, H, W, lanes, 'fg_hist_refine')
    _chk(q, dtype=torch.uint8, name='fg_hist_refine: q')
    lo = torch.as_tensor(lo, dtype=torch.float32).reshape(-1).contiguous()
    scale = torch.as_tensor(scale, dtype=torch.float32).reshape(-1).contiguous()
    if lo.is_cuda or scale.is_cuda or lo.numel() != 3 or scale.numel() != 3:
        raise ValueError('fg_hist_refine: lo and scale are host triples (fg_colour_params)')
    dev = x.device
    nb = bins ** 3
    F = torch.empty((B, nb), dtype=torch.int32, device=dev)
    N = torch.empty((B, nb), dtype=torch.int32, device=dev)
    s = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    idx = workspace(B * T * ((H * W + 3) // 4 * 4) * 2, dev, 'fg_idx')
    check(lib().bdv_fg_hist_refine(_p(x), _p(q), B, T, H, W, code, bins, ctypes.c_void_p(lo.data_ptr()), ctypes.c_void_p(scale.data_ptr()),
                                   _p(idx), _p(F), _p(N), _p(s), _stream()), 'bdv_fg_hist_refine')
    return s, F, N


def fg_select(s, k_fg: int):
    """Stage 6 (``bdv_fg_select``): ``s`` (B, H, W) or (B, HW) non-negative fp32 -> ``(v (B,), mask uint8 like s, count int32 (B,))``."""
    if not isinstance(s, torch.Tensor) or s.dim() not in (2, 3) or s.numel() == 0:
        raise ValueError(f'fg_select: expected a non-empty (B, H, W) or (B, HW) map, got {tuple(getattr(s, "shape", ()))}')
    B, HW = int(s.shape[0]), s.numel() // int(s.shape[0])
    k_fg = int(k_fg)
    if not 1 <= k_fg <= HW or HW > 1 << 24:
        raise ValueError(f'fg_select: k_fg {k_fg} outside 1..{HW} (H * W <= 2^24)')
    _chk(s, name='fg_select: s')
    v = torch.empty((B,), dtype=torch.float32, device=s.device)
    mask = torch.empty(s.shape, dtype=torch.uint8, device=s.device)
    count = torch.empty((B,), dtype=torch.int32, device=s.device)
    check(lib().bdv_fg_select(_p(s), B, HW, k_fg, _p(v), _p(mask), _p(count), _stream()), 'bdv_fg_select')
    return v, mask, count


def fg_merge_slots(perm, apply):
    """Host side of stage 7: a scratch slot for every clip whose source may itself be merged.  -> (slot int32 (B,) host, nslots)."""
    perm, apply = perm.tolist(), [bool(a) for a in apply.tolist()]
    on = [apply[b] and perm[b] != b for b in range(len(perm))]
    slot, n = [], 0
    for b in range(len(perm)):
        if on[b] and on[perm[b]]:
            slot.append(n)
            n += 1
        else:
            slot.append(-1)
    return torch.tensor(slot, dtype=torch.int32), n


def fg_merge_(x, mask, count, perm, apply, B, T, H, W, layout='tchw'):
    """Stage 7 (``bdv_fg_merge``), in place: the background (``mask == 0``) of every clip b with ``apply[b]``, ``perm[b] != b`` and
    ``count[b] > 0`` takes the pixels clip ``perm[b]`` had before the call.  ``perm``: host int64 (B,), ``apply``: host bool (B,).
    Returns ``x``."""
    B, T, H, W, code, lanes = _fg_dims(B, T, H, W, layout, 'fg_merge_')
    if not isinstance(mask, torch.Tensor) or mask.numel() != B * H * W:
        raise ValueError(f'fg_merge_: mask {tuple(getattr(mask, "shape", ()))} does not fit {B} clips of {H} x {W} pixels')
    _fg_clip(x, B, T, H, W, lanes, 'fg_merge_')
    _chk(mask, dtype=torch.uint8, name='fg_merge_: mask')
    _chk(count, (B,), torch.int32, 'fg_merge_: count')
    perm_dev = _blend_perm(perm, B, x.device, 'fg_merge_')
    host_perm = torch.as_tensor(perm, dtype=torch.int64).reshape(-1)
    apply = torch.as_tensor(apply).reshape(-1)
    if apply.is_cuda or apply.numel() != B:
        raise ValueError(f'fg_merge_: apply must be a host vector of {B} flags')
    apply = apply.to(torch.bool)
    slot, nslots = fg_merge_slots(host_perm, apply)
    S = T * H * W * lanes
    ws = workspace(nslots * S * 4, x.device, 'fg_merge') if nslots else None
    apply_dev, slot_dev = apply.to(torch.uint8).to(x.device), slot.to(x.device)      # both alive until the launches are queued
    check(lib().bdv_fg_merge(_p(x), _p(mask), _p(count), _p(perm_dev), _p(apply_dev), _p(slot_dev), nslots,
                             B, T, H, W, code, _p(ws), 0 if ws is None else ws.numel(), _stream()), 'bdv_fg_merge')
    return x
