"""Time-channel importance for the feature distillation of ``methods='base'`` (config key ``kd_importance``).

UPSTREAM TCD (Park, Kang, Han, "Class-Incremental Learning for Action Recognition in Videos", ICCV 2021) -- not in the reference,
restated as DESIGN 4.12 defines it, parity unpinned.  After task k the squared per-sample gradient of the classification loss at every
distilled module is summed per (segment, channel) over the task's training records; the normalised map (mean 1) is averaged with the
earlier tasks' maps and weights the MSE of libs/cil/cil.py:519-541 during task k + 1 (``functional.kd_time_channel``).  The sum runs
in csrc/tc_kd.hip (``kernels.tc_sqgrad_accum``); this file holds the estimator around it and the map arithmetic.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch

from . import kernels as K
from .gradcam import _ReRoot, borrowed_frozen_eval
from .hooks import rgetattr

KD_IMPORTANCE_TYPES = ('time_channel',)


def update_kd_importance(S: torch.Tensor, count, prev: Optional[torch.Tensor], task: int, mix: float = 0.0
                         ) -> Tuple[torch.Tensor, torch.Tensor, bool]:
    """Normalise, merge and mix one module's map.  ``S`` (T, C): the summed squared per-sample gradients, ``count``: the samples,
    ``prev``: the unmixed map after task ``task - 1`` (None for task 0).

        raw = S / count;  A^ = raw / mean(raw)  (all ones when mean(raw) is 0 or not finite)
        A_k = (k * A_{k-1} + A^) / (k + 1), A_0 = A^;   mixed = (1 - mix) * A_k + mix

    Returns ``(A_k, mixed, degenerate)``: fp32 CPU tensors -- ``A_k`` is what the next task merges from and what the file stores,
    ``mixed`` is what the distillation uses -- and whether the all-ones fallback was taken.  Pure: no GPU, no state."""
    if not 0.0 <= float(mix) <= 1.0:
        raise ValueError(f'kd_importance: mix must be in [0, 1], got {mix!r}')
    if task < 0 or (task > 0 and prev is None):
        raise ValueError(f'kd_importance: task {task} needs the map of task {task - 1}')
    raw = S.detach().to('cpu', torch.float64) / float(count) if float(count) > 0 else torch.full(S.shape, float('nan'), dtype=torch.float64)
    mean = raw.mean()
    degenerate = not bool(torch.isfinite(raw).all()) or not bool(torch.isfinite(mean)) or float(mean) <= 0.0
    new = torch.ones_like(raw) if degenerate else raw / mean
    if task > 0:
        p = prev.detach().to('cpu', torch.float64)
        if p.shape != new.shape:
            raise ValueError(f'kd_importance: the map of task {task - 1} has shape {tuple(p.shape)}, this task gives {tuple(new.shape)}')
        new = (task * p + new) / (task + 1)
    mixed = (1.0 - float(mix)) * new + float(mix)
    return new.to(torch.float32), mixed.to(torch.float32), degenerate


def _tap_channels(t: torch.Tensor) -> int:
    return int(t.shape[1])


def estimate_kd_importance(model, batches: Iterable[Dict], module_names: Sequence[str], num_segments: int
                           ) -> Dict[str, Tuple[torch.Tensor, int]]:
    """``{name: (S, count)}``: for every batch ``dict(imgs=, label=)`` the classification loss ``loss_cls`` on the true labels, its
    gradient g at each named module's output, and ``S[t, c] += sum_{b,h,w} (B * g[b*T+t, c, h, w])^2``, ``count += B`` -- the loss is a
    batch mean and eval-mode rows are independent, so ``B * g`` is the per-sample gradient.

    The model is borrowed as ``GradCAM`` borrows it: eval mode, every parameter frozen (no weight gradient is computed), and mode
    flags, ``requires_grad`` flags and ``test_cfg`` are as before afterwards, also when the forward raises.  Every named module is
    tapped with a forward hook; the first one the forward reaches carries no graph and is re-rooted as a leaf, the later ones hang
    off it.  Each gradient goes to ``kernels.tc_sqgrad_accum`` and is dropped.  ``S`` is fp32 (T, C) on the model's device."""
    from .resnet3d import Recognizer3D
    if isinstance(model, Recognizer3D):
        raise NotImplementedError('estimate_kd_importance: Recognizer3D is not supported (2D recognizers only: rows must be frames)')
    if K.get_conv_arith() == 'bf16':
        raise NotImplementedError("estimate_kd_importance: the 'bf16' conv arithmetic stores activations in bf16, which has no eval-mode "
                                  "backward; use set_conv_arith('bf16x1') for bf16 products on fp32 tensors")
    names = list(module_names)
    if not names or len(set(names)) != len(names):
        raise ValueError(f'estimate_kd_importance: module_names must be distinct and not empty, got {names}')
    T = int(num_segments)
    if T <= 0:
        raise ValueError(f'estimate_kd_importance: num_segments must be positive, got {num_segments!r}')
    modules = []
    for n in names:
        try:
            m = rgetattr(model, n)
        except AttributeError:
            raise AttributeError(f'Module {n} not found') from None
        modules.append(m)
    taps = [_ReRoot(dims=(2, 4), who=f'estimate_kd_importance: module {n}', expected='an (N, C, h, w) or (N, D) tensor') for n in names]
    acc: Dict[str, torch.Tensor] = {}
    count = 0
    with borrowed_frozen_eval(model):
        handles = [m.register_forward_hook(tap) for m, tap in zip(modules, taps)]
        try:
            for batch in batches:
                imgs, labels = batch['imgs'], batch['label']
                B = int(labels.shape[0])
                for tap in taps:
                    tap.output = None
                with torch.enable_grad():
                    losses = model.forward_train(imgs, labels, batch_data=batch)      # not model(...): no train_cfg.blending here
                    outs = [tap.output for tap in taps]
                    for n, o in zip(names, outs):
                        if o is None:
                            raise RuntimeError(f'estimate_kd_importance: the forward pass never ran {n}')
                        if o.shape[0] != B * T:
                            raise ValueError(f'estimate_kd_importance: {n} returned {o.shape[0]} rows for {B} clips x {T} segments')
                    grads = torch.autograd.grad(losses['loss_cls'], outs)
                del losses
                for n, o, g in zip(names, outs, grads):
                    if n not in acc:
                        acc[n] = torch.zeros((T, _tap_channels(o)), dtype=torch.float32, device=o.device)
                    K.tc_sqgrad_accum(acc[n], g, float(B))
                del grads, outs
                count += B
        finally:
            for h in handles:
                h.remove()
            for tap in taps:
                tap.output = None
    return {n: (acc[n], count) for n in names if n in acc}
