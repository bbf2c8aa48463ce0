"""Grad-CAM for the 2D recognizers: where in the frames does a class score come from?

UPSTREAM mmaction2 ``GradCAM`` (mmaction/utils/gradcam_utils.py, used by demo/demo_gradcam.py) -- not vendored, restated from memory,
parity unpinned.  ``_calculate_localization_map`` for a 2D recognizer: the model in ``eval()``, ``test_cfg['average_clips'] =
'score'``, ``preds = model(imgs, return_loss=False)``, the label's logit (or the row maximum) summed over the batch, its gradient
with respect to the target layer's activation, channel weights = the gradient's spatial mean, map = relu(sum_c w_c A_c), bilinear
upsampling to the input size, min-max normalisation per sample (all T frames of a clip share one minimum and maximum, delta 1e-20).
The arithmetic after the backward pass runs in csrc/gradcam.hip.

Deliberate differences from upstream:
  * the gradient is taken with ``torch.autograd.grad(score_sum, [activation])`` instead of ``zero_grad()`` + ``backward()``: no
    parameter's ``.grad`` is touched.  Every parameter's ``requires_grad`` is switched off for the call (and restored), so the
    autograd nodes, which consult ``needs_input_grad``, compute no weight gradient at all, and the activation is re-rooted at the tap
    (``detach().requires_grad_()``) -- a model frozen by ``freeze_backbone()`` or ``frozen_stages=4`` gives the same map as an unfrozen
    one, bit for bit;
  * module ``training`` flags, ``test_cfg`` and the ``requires_grad`` flags are restored afterwards, also when the call raises;
  * besides the map the call can return the colormap overlay and, given per-frame boxes, the share of the map inside them.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import numpy as np
import torch

from . import functional as Fn
from . import kernels as K
from .frontend import IMG_MEAN, IMG_STD
from .hooks import rgetattr
from .resnet_tsm import Nhwc4Frames


def builtin_colormap() -> np.ndarray:
    """The (256, 3) float32 table used when no colormap is given: the piecewise-linear "jet" ramps r, g, b =
    clamp(1.5 - |4x - 3|), clamp(1.5 - |4x - 2|), clamp(1.5 - |4x - 1|) at x = (i + 0.5) / 256."""
    x = (np.arange(256, dtype=np.float64) + 0.5) / 256.0
    rgb = np.stack([1.5 - np.abs(4.0 * x - c) for c in (3.0, 2.0, 1.0)], axis=1)
    return np.clip(rgb, 0.0, 1.0).astype(np.float32)


def check_colormap(lut) -> np.ndarray:
    """A caller's table as (256, 3) float32 in [0, 1] (e.g. ``matplotlib.cm.viridis(np.arange(256))[:, :3]``)."""
    a = np.asarray(lut.detach().cpu() if isinstance(lut, torch.Tensor) else lut, dtype=np.float32)
    if a.shape != (256, 3):
        raise ValueError(f'colormap: expected a (256, 3) table, got shape {a.shape}')
    if not np.isfinite(a).all() or a.min() < 0.0 or a.max() > 1.0:
        raise ValueError(f'colormap: values must lie in [0, 1], got [{a.min()}, {a.max()}]')
    return np.ascontiguousarray(a)


def colormap_index(v) -> np.ndarray:
    """The table row of a normalised value: ``min(255, floor(256 * v))`` (matplotlib's ``Colormap.__call__`` for floats in [0, 1])."""
    return np.minimum(255, np.floor(256.0 * np.asarray(v, dtype=np.float64))).astype(np.int64)


def box_table(boxes, B: int, T: int):
    """Per-frame boxes -> the CSR pair ``(offsets (B*T + 1,) int64, rows (n, 4) float32)`` of ``bdv_gradcam_render`` (built like
    ``actor_cut_mix.acm_plan_table`` builds its tables).  ``boxes``: B clips x T frames of (n, 4) arrays ``x0 y0 x1 y1`` in output-pixel
    coordinates, or such a pair already."""
    if isinstance(boxes, tuple) and len(boxes) == 2 and not isinstance(boxes[0], (list, tuple)):
        off = np.asarray(boxes[0]).reshape(-1)
        rows = np.asarray(boxes[1], dtype=np.float32)
        return off, rows.reshape(-1, 4) if rows.size == 0 else rows
    if len(boxes) != B or any(len(c) != T for c in boxes):
        raise ValueError(f'boxes: expected {B} clips of {T} frames each')
    frames = [np.asarray(f, dtype=np.float32).reshape(-1, 4) for c in boxes for f in c]
    off = np.zeros(len(frames) + 1, np.int64)
    off[1:] = np.cumsum([len(f) for f in frames])
    return off, (np.concatenate(frames) if frames else np.zeros((0, 4), np.float32))


class _ReRoot:
    """Forward hook of the target module: keeps its output, re-rooted as a leaf when it carries no graph (every parameter frozen).
    ``dims``: the tensor ranks the module may return; ``who``: the caller, for the message."""

    def __init__(self, dims=(4,), who='GradCAM: the target layer', expected='an (N, C, h, w) tensor'):
        self.output = None
        self.dims, self.who, self.expected = tuple(dims), who, expected

    def __call__(self, module, inputs, output):
        if not isinstance(output, torch.Tensor) or output.dim() not in self.dims:
            raise TypeError(f'{self.who} must return {self.expected}, got {type(output).__name__} '
                            f'{tuple(getattr(output, "shape", ()))}')
        if not output.requires_grad:
            output = output.detach().requires_grad_()
        self.output = output
        return output


@contextlib.contextmanager
def borrowed_frozen_eval(model):
    """eval mode, ``average_clips='score'``, no trainable parameter -- and everything as it was afterwards, also when the body
    raises.  Shared by ``GradCAM`` and ``kd_importance.estimate_kd_importance``."""
    flags = [(m, m.training) for m in model.modules()]
    grads = [(p, p.requires_grad) for p in model.parameters()]
    had_cfg = hasattr(model, 'test_cfg')
    cfg = model.test_cfg if had_cfg else None
    try:
        model.eval()
        model.test_cfg = dict(cfg or {}, average_clips='score')
        for p, _ in grads:
            p.requires_grad_(False)
        yield
    finally:
        for p, r in grads:
            p.requires_grad_(r)
        if had_cfg:
            model.test_cfg = cfg
        else:
            del model.test_cfg
        for m, t in flags:
            m.training = t


class GradCAM:
    """``GradCAM(model, target_layer='backbone.layer4')(imgs, labels)`` -> dict with ``map`` (B, T, H, W) fp32 in [0, 1], ``preds``
    (B, K), ``labels`` (B,) int64 -- the class each clip's score was taken from: the given labels, or the row maximum of ``preds`` when
    none were given -- and on request ``overlay`` (B, T, H, W, 3) uint8 and ``actor_attention`` (B,).

    ``target_layer``: a dotted module path as ``OutputHook`` takes it (``backbone.layer1`` .. ``backbone.layer4``, or a block such as
    ``backbone.layer4.1``) whose output is (N, C, h, w).  ``colormap``: a (256, 3) table in [0, 1]; None = ``builtin_colormap()``.
    ``mean`` / ``std``: the ``Normalize`` the input went through (the overlay de-normalises the model's own input)."""

    def __init__(self, model, target_layer: str = 'backbone.layer4', colormap=None, mean=IMG_MEAN, std=IMG_STD):
        from .resnet3d import Recognizer3D
        if isinstance(model, Recognizer3D):
            raise NotImplementedError('GradCAM: Recognizer3D is not supported (2D recognizers only: the map is taken per frame)')
        try:
            self.target = rgetattr(model, target_layer)
        except AttributeError:
            raise AttributeError(f'Module {target_layer} not found') from None
        if not isinstance(self.target, torch.nn.Module):
            raise AttributeError(f'{target_layer} is not a module')
        self.model, self.target_layer = model, target_layer
        self.lut = builtin_colormap() if colormap is None else check_colormap(colormap)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self._lut_dev = None

    def _borrowed(self):
        """eval mode, ``average_clips='score'``, no trainable parameter -- and everything as it was afterwards."""
        return borrowed_frozen_eval(self.model)

    def _forward(self, imgs):
        return self.model(imgs, return_loss=False)

    def __call__(self, imgs, labels=None, *, boxes=None, alpha: float = 0.5, overlay: bool = False):
        if K.get_conv_arith() == 'bf16':
            raise NotImplementedError("GradCAM: the 'bf16' conv arithmetic stores activations in bf16, which has no eval-mode backward; "
                                      "use set_conv_arith('bf16x1') for bf16 products on fp32 tensors")
        if isinstance(imgs, Nhwc4Frames):
            B, T, _, H, W = imgs.shape
            dev = imgs.data.device
        else:
            if not isinstance(imgs, torch.Tensor) or imgs.dim() != 5 or imgs.shape[2] != 3:
                raise ValueError(f'GradCAM: imgs must be (B, T, 3, H, W) or Nhwc4Frames, got {tuple(getattr(imgs, "shape", ()))}')
            B, T, _, H, W = (int(d) for d in imgs.shape)
            dev = imgs.device
        segs = getattr(getattr(self.model, 'cls_head', None), 'num_segments', None)
        if segs is not None and T != segs:
            raise ValueError(f'GradCAM: imgs.shape[1] = {T} but cls_head.num_segments = {segs}: only one clip per sample is supported '
                             '(no multi-clip / multi-crop inputs)')
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f'GradCAM: alpha {alpha} outside [0, 1]')
        if labels is not None:
            labels = torch.as_tensor(labels).reshape(-1).to(dev, torch.int64)
            if labels.numel() != B:
                raise ValueError(f'GradCAM: {labels.numel()} labels for {B} clips')
        table = box_table(boxes, B, T) if boxes is not None else None

        tap = _ReRoot()
        with self._borrowed():
            handle = self.target.register_forward_hook(tap)
            try:
                with torch.enable_grad():
                    preds = self._forward(imgs)
                    if preds.dim() != 2 or preds.shape[0] != B:
                        raise ValueError(f'GradCAM: the model returned scores of shape {tuple(preds.shape)} for {B} clips')
                    if labels is not None and (int(labels.min()) < 0 or int(labels.max()) >= preds.shape[1]):
                        raise ValueError(f'GradCAM: labels outside [0, {preds.shape[1]})')
                    pick = preds.detach().argmax(dim=1) if labels is None else labels
                    score = preds.gather(1, pick.view(-1, 1)).sum()
                    act = tap.output
                    if act is None:
                        raise RuntimeError(f'GradCAM: the forward pass never ran {self.target_layer}')
                    (grad,) = torch.autograd.grad(score, [act])
            finally:
                handle.remove()
        if act.shape[0] != B * T:
            raise ValueError(f'GradCAM: {self.target_layer} returned {act.shape[0]} frames for {B} x {T}')
        a = Fn.nchw_view_to_nhwc(act.detach())
        g = Fn.nchw_view_to_nhwc(grad)
        if a.dtype != torch.float32 or g.dtype != torch.float32:
            raise TypeError(f'GradCAM: fp32 activations expected, got {a.dtype} / {g.dtype}')
        m = K.gradcam_map(a, K.avgpool_fwd(g))
        mm = K.gradcam_minmax(m, B, T, H, W)
        frames4 = lut = None
        if overlay:
            frames4 = imgs.data if isinstance(imgs, Nhwc4Frames) else K.nchw3_to_nhwc4(imgs.detach().reshape(B * T, 3, H, W).contiguous())
            if self._lut_dev is None or self._lut_dev.device != dev:
                self._lut_dev = torch.from_numpy(self.lut).to(dev)
            lut = self._lut_dev
        v, ov, sums = K.gradcam_render(m, mm, B, T, H, W, True, frames4, lut, alpha, self.mean, self.std,
                                       None if table is None else table[0], None if table is None else table[1])
        out = {'map': v, 'preds': preds.detach(), 'labels': pick}
        if overlay:
            out['overlay'] = ov
        if table is not None:
            off = torch.as_tensor(np.asarray(table[0], dtype=np.int64))
            has_box = (off[T::T] - off[:-1:T]) > 0                      # per clip: a box in any of its frames
            out['actor_attention'] = actor_attention_ratio(sums, has_box)
        return out


def actor_attention_ratio(sums: torch.Tensor, has_box: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 2) box sums of ``bdv_gradcam_render`` -> (B,) share of the map inside the boxes; nan where the map is empty or, with
    ``has_box`` (B,) bool, where the clip has no box."""
    ok = sums[:, 0] > 0
    if has_box is not None:
        ok = ok & has_box.to(sums.device)
    return torch.where(ok, sums[:, 1] / sums[:, 0], torch.full_like(sums[:, 0], float('nan')))
