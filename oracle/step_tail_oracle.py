"""CPU oracle for the tail of a training step -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

What a step runs after the average pool -- csrc/head_loss.hip (LSC / linear heads, consensus, LSCLoss, soft and plain cross entropy,
iCaRL / ActorCutMix targets, feature-KD MSE) and csrc/optim.hip (squared norm, clip coefficient, SGD step) -- restated in plain
torch on top of oracle/tsm_oracle.py.  Every function computes in the dtype of its tensor inputs: fp64 copies of the fp32 inputs give
the high-precision reference that tests/test_head_edges_gpu.py, test_loss_edges_gpu.py and test_optim_edges_gpu.py hold the kernels
against, fp32 inputs give torch's own fp32 arithmetic, and the distance between the two runs is what the tests' bars are built from
(``bar``).  Scalars that a kernel receives as a C ``float`` (margin, lr, weight decay, momentum, grad scale, max norm) enter the fp64
run at their fp32 value (``f32``): they are inputs, not arithmetic.

The case tables of the three GPU files and the functions that draw their inputs live here as well, so that
tests/test_step_tail_cpu.py can check, without a GPU, that every case meets its margin condition and has a finite positive bar.

Pinning: tests/test_step_tail_cpu.py holds ``lsc_head`` / ``linear_head`` / ``lsc_loss`` / ``acm_soft_ce`` against the goldens made
from the reference's own files (head_loss_golden.npz, lsc_weights_golden.npz, acm_golden.npz) and ``sgd_step`` / ``clip_coef``
against torch.optim.SGD + clip_grad_norm_.
"""
import functools
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import tsm_oracle as O

U = 2.0 ** -24              # fp32 unit roundoff
COS_EPS = 1e-8              # F.cosine_similarity's eps, COS_EPS of csrc/head_loss.hip
MARGIN = 1e-4               # what an fp64 decision (arg-max, hinge) must be decided by for fp32 not to flip it

FLOOR_SUM = 2e-7            # plain sums and dot products
FLOOR_FN = 2e-6             # anything through a division, expf, logf, sqrtf or powf
CAP_FWD = (1e-5, 1e-6)      # tests/test_ops_gpu.py::_close for forward values: tol * scale + atol
CAP_GRAD = (1e-4, 1e-7)     # ... and for gradients
CAP_GRAD5 = (1e-5, 1e-7)    # ... and where it compares a gradient at 1e-5 (linear head, soft cross entropy)
CAP_TGT = (1e-6, 1e-6)      # ... ActorCutMix targets


def f32(v) -> float:
    """The value a C ``float`` argument carries."""
    return float(np.float32(v))


def bar(ref64: torch.Tensor, ref32: torch.Tensor, floor: float, *caps) -> float:
    """floor * max(1, scale) + 4 x the largest deviation of the fp32 run from the fp64 run, no looser than any of ``caps``
    ((rel, abs) -> rel * scale + abs); scale = max |ref64|.  Built from the two references only."""
    ref64, ref32 = torch.as_tensor(ref64, dtype=torch.float64), torch.as_tensor(ref32).double()
    assert ref64.shape == ref32.shape, (ref64.shape, ref32.shape)
    scale = ref64.abs().max().item() if ref64.numel() else 0.0
    dev = torch.nan_to_num((ref32 - ref64).abs(), nan=0.0).max().item() if ref64.numel() else 0.0
    b = floor * max(1.0, scale) + 4.0 * dev
    for rel, ab in caps:
        b = min(b, rel * scale + ab)
    return b


def _leaf(t, dtype=None):
    return t.detach().clone().to(dtype or t.dtype).requires_grad_(True)


# ---- heads ---------------------------------------------------------------------------------------------------------------

LSC_CASES = [(1, 1, 1, 1), (3, 7, 2, 3), (4, 64, 5, 1), (5, 63, 37, 3), (9, 257, 101, 1), (2, 65, 300, 2), (5, 2048, 101, 10),
             (4, 2048, 851, 2)]                       # the last one: 4 * (D + K*P) * 4 = 60000 bytes of LDS, the limit exactly
LINEAR_CASES = [(1, 1, 1), (3, 7, 2), (4, 64, 8), (5, 63, 9), (9, 257, 101), (7, 2048, 101), (2, 65, 300), (1875, 5, 3)]
CONSENSUS_CASES = [(1, 1, 1), (3, 8, 37), (5, 3, 300)]


def lsc_head(x, w, K, P, dsim=None):
    """cosine_linear.py:27-43 with the saved tensors of ``bdv_lsc_fwd``: sim (N, K), xnorm (N,), wnorm (K*P,), cosbuf (N, K*P), and
    with ``dsim`` the autograd gradients dx, dw.  ``F.cosine_similarity`` spelled out: each norm is clamped at eps on its own."""
    x, w = _leaf(x), _leaf(w)
    wm = w.reshape(K * P, x.shape[1])
    xn = x.norm(dim=1).clamp_min(COS_EPS)
    wn = wm.norm(dim=1).clamp_min(COS_EPS)
    cos = (x @ wm.t()) / (xn[:, None] * wn[None, :])
    pc = cos.reshape(-1, K, P)
    sim = (torch.softmax(pc, dim=2) * pc).sum(dim=2)
    out = dict(sim=sim.detach(), xnorm=xn.detach(), wnorm=wn.detach(), cosbuf=cos.detach())
    if dsim is not None:
        out['dx'], out['dw'] = torch.autograd.grad(sim, (x, w), dsim.to(sim.dtype))
    return out


def linear_head(x, w, b=None, dout=None):
    """inc_net.py:36-37: out = x w^T + b, and with ``dout`` the autograd gradients dx, dw, db."""
    x, w = _leaf(x), _leaf(w)
    b = None if b is None else _leaf(b)
    res = F.linear(x, w, b)
    out = dict(out=res.detach())
    if dout is not None:
        leaves = (x, w) if b is None else (x, w, b)
        grads = torch.autograd.grad(res, leaves, dout.to(res.dtype))
        out.update(zip(('dx', 'dw', 'db'), grads))
    return out


def head_input(kind, ci):
    """fp32 inputs of LSC case ``ci`` (x, w, dsim, K, P) or linear case ``ci`` (x, w, b, dout): signed, at the sizes of a head (weights
    about 1/sqrt(D), an upstream gradient of about 1/N)."""
    g = torch.Generator().manual_seed((3000 if kind == 'lsc' else 3100) + ci)
    if kind == 'lsc':
        N, D, K, P = LSC_CASES[ci]
        return (torch.randn(N, D, generator=g), torch.randn(K, P * D, generator=g) / math.sqrt(D),
                torch.randn(N, K, generator=g) / N, K, P)
    N, D, K = LINEAR_CASES[ci]
    return (torch.randn(N, D, generator=g), torch.randn(K, D, generator=g) / math.sqrt(D), torch.randn(K, generator=g),
            torch.randn(N, K, generator=g) / N)


@functools.lru_cache(maxsize=None)
def lsc_case(ci):
    """(inputs, fp64 run, bars) of LSC case ``ci``."""
    x, w, dsim, K, P = head_input('lsc', ci)
    r64 = lsc_head(x.double(), w.double(), K, P, dsim.double())
    r32 = lsc_head(x, w, K, P, dsim)
    bars = {k: bar(r64[k], r32[k], FLOOR_FN, CAP_FWD) for k in ('sim', 'xnorm', 'wnorm', 'cosbuf')}
    bars.update({k: bar(r64[k], r32[k], FLOOR_FN, CAP_GRAD) for k in ('dx', 'dw')})
    return (x, w, dsim, K, P), r64, bars


@functools.lru_cache(maxsize=None)
def linear_case(ci, with_bias):
    x, w, b, dout = head_input('linear', ci)
    b = b if with_bias else None
    r64 = linear_head(x.double(), w.double(), None if b is None else b.double(), dout.double())
    r32 = linear_head(x, w, b, dout)
    bars = dict(out=bar(r64['out'], r32['out'], FLOOR_SUM, CAP_FWD))
    bars.update({k: bar(r64[k], r32[k], FLOOR_SUM, CAP_GRAD, CAP_GRAD5) for k in r64 if k != 'out'})
    return (x, w, b, dout), r64, bars


def dyadic(shape, g, lo=-16, hi=17):
    """Multiples of 1/8 in [-2, 2]: sums of a few of them are exact in fp32."""
    return torch.randint(lo, hi, shape, generator=g).float() / 8


def consensus(s, B, T):
    return s.reshape(B, T, -1).mean(dim=1)


def consensus_grad(dout, T):
    return (dout / T)[:, None, :].expand(-1, T, -1).reshape(dout.shape[0] * T, -1)


# ---- LSCLoss -------------------------------------------------------------------------------------------------------------

LOSS_BK = [(1, 1), (3, 5), (4, 64), (5, 65), (6, 101), (9, 300), (130, 37)]
ETAS = [0.37, 1.0, 10.0]
LOSS_MARGINS = [0.0, 0.6]
WEIGHTS = ['none', 'positive', 'negative']
LSC_LOSS_CASES = list(itertools.product(range(len(LOSS_BK)), ETAS, LOSS_MARGINS, (False, True), WEIGHTS))


def lsc_loss(sim, targets, eta, margin=0.6, hinge=True, class_weights=None):
    """lsc_loss.py:36-56 (exclude_pos_denominator=True; oracle/tsm_oracle.py::lsc_loss) with ``class_weights`` (:50-51): the weight
    multiplies num - log(den) BEFORE the negation and the hinge.  Returns the loss, its autograd gradients dsim and deta (the row
    maximum is not detached in the reference: its arg-max takes 1/den), the rows' values before the hinge and eta * (sim - margin)."""
    sim = _leaf(sim)
    eta = _leaf(eta.reshape(1), sim.dtype)
    s0 = eta * (sim - f32(margin))
    s = s0 - s0.max(dim=1, keepdim=True)[0]
    idx = torch.arange(s.shape[0])
    num = s[idx, targets]
    den = s.clone()
    den[idx, targets] = 0.0
    rows = num - torch.log(torch.exp(den).sum(-1))
    if class_weights is not None:
        rows = class_weights.to(sim.dtype)[targets] * rows
    rows = -rows
    loss = (torch.clamp(rows, min=0.0) if hinge else rows).mean()
    dsim, deta = torch.autograd.grad(loss, (sim, eta))
    return dict(loss=loss.detach(), dsim=dsim, deta=deta, rows=rows.detach(), s=s0.detach())


def top2_gap(s):
    """Per row: largest minus second largest value; inf for a single column."""
    if s.shape[1] < 2:
        return torch.full((s.shape[0],), float('inf'), dtype=torch.float64)
    top = s.double().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def lsc_loss_margin_ok(ref64, B, K, hinge, wkind):
    """The margin condition of a drawn case, from its fp64 run: every row's arg-max is decided by MARGIN; with the hinge on every row's
    value is MARGIN away from zero; with a negative weight there is a row on either side of zero (``one row`` cannot have both, and a
    single class gives every row the value 0 exactly, in any precision: those two are exempt from the last two conditions)."""
    if top2_gap(ref64['s']).min().item() < MARGIN:
        return False
    rows = ref64['rows']
    if K > 1 and hinge and rows.abs().min().item() < MARGIN:
        return False
    if K > 1 and B > 1 and wkind == 'negative' and not ((rows > 0).any() and (rows < 0).any()):
        return False
    return True


def draw_lsc_loss(B, K, wkind, seed):
    g = torch.Generator().manual_seed(seed)
    sim = torch.rand(B, K, generator=g) * 2 - 1
    targets = torch.randint(0, K, (B,), generator=g)
    cw = None
    if wkind != 'none':
        cw = torch.rand(K, generator=g) * 1.5 + 0.25
        if wkind == 'negative':
            cw[targets[0]] = -0.75
    return sim, targets, cw


@functools.lru_cache(maxsize=None)
def lsc_loss_case(case):
    """(inputs, t, fp64 run, bars) of LSC_LOSS_CASES[case]: the first of the seeds 20000 + 100 * case + t, t in range(20), whose fp64
    run meets ``lsc_loss_margin_ok``.  No case is dropped: finding none is an error."""
    bi, eta, margin, hinge, wkind = LSC_LOSS_CASES[case]
    B, K = LOSS_BK[bi]
    eta_t = torch.tensor([eta], dtype=torch.float32)
    for t in range(20):
        sim, targets, cw = draw_lsc_loss(B, K, wkind, 20000 + 100 * case + t)
        r64 = lsc_loss(sim.double(), targets, eta_t.double(), margin, hinge, None if cw is None else cw.double())
        if lsc_loss_margin_ok(r64, B, K, hinge, wkind):
            r32 = lsc_loss(sim, targets, eta_t, margin, hinge, cw)
            bars = dict(loss=bar(r64['loss'], r32['loss'], FLOOR_FN, CAP_FWD),
                        dsim=bar(r64['dsim'], r32['dsim'], FLOOR_FN, CAP_GRAD),
                        deta=bar(r64['deta'], r32['deta'], FLOOR_FN, CAP_GRAD))
            return (sim, targets, eta_t, cw), t, r64, bars
    raise AssertionError(f'no seed in 20 gives lsc_loss case {LSC_LOSS_CASES[case]} its margins')


# ---- soft / plain cross entropy and the target builders --------------------------------------------------------------------

SOFT_KINDS = ['labels', 'onehot', 'acm', 'softmax', 'sum0.7']
SCORE_SCALES = [1.0, 80.0]           # 80: expf overflows unless the row maximum is subtracted


def soft_ce(score, targets=None, labels=None):
    """icarl.py:123-125 on a target table (oracle/tsm_oracle.py::soft_target_ce), or plain mean cross entropy on integer labels:
    loss and its autograd gradient."""
    score = _leaf(score)
    loss = O.soft_target_ce(score, targets.to(score.dtype)) if targets is not None else F.cross_entropy(score, labels)
    return dict(loss=loss.detach(), dscore=torch.autograd.grad(loss, score)[0])


def acm_targets(labels, bg, fg_ratio, alpha, K):
    """acm_smooth_ce.py:18-28: onehot(label) * lam + (1 - lam) * onehot(bg), lam = 1 - (1 - fg)^alpha, background -1 -> class 0;
    in the dtype of ``fg_ratio``."""
    dt = fg_ratio.dtype
    bg = bg.clone()
    bg[bg == -1] = 0
    lam = (1 - (1 - fg_ratio) ** f32(alpha)).reshape(-1, 1)
    return F.one_hot(labels, K).to(dt) * lam + (1 - lam) * F.one_hot(bg, K).to(dt)


def acm_soft_ce(score, labels, bg, fg_ratio, alpha):
    """ACMSmoothCE as the project applies it: the soft cross entropy of ``acm_targets`` (the reference's sum has no negation:
    oracle/tsm_oracle.py::acm_smooth_ce is minus this)."""
    return soft_ce(score, acm_targets(labels, bg.reshape(-1), fg_ratio.reshape(-1).to(score.dtype), alpha, score.shape[1]))


def icarl_targets(labels, K, prev_logits, prev_K, base=None):
    """icarl.py:101-120: ``base`` (or one-hot) rows, rows of old-class samples replaced by softmax(prev logits); in the dtype of
    ``prev_logits`` / ``base`` (fp64 when both are missing)."""
    dt = prev_logits.dtype if prev_logits is not None else base.dtype if base is not None else torch.float64
    tgt = F.one_hot(labels, K).to(dt) if base is None else base.clone().to(dt)
    if prev_logits is not None:
        old = labels < prev_K
        tgt[old] = torch.softmax(prev_logits[old], dim=1)
    return tgt


def softce_input(bi, kind, scale):
    """(score, soft targets or None, labels or None) of one soft-CE case, fp32."""
    B, K = LOSS_BK[bi]
    g = torch.Generator().manual_seed(21000 + 100 * bi + 10 * SOFT_KINDS.index(kind) + int(scale > 1))
    score = (torch.rand(B, K, generator=g) * 2 - 1) * scale if scale > 1 else torch.randn(B, K, generator=g)
    labels = torch.randint(0, K, (B,), generator=g)
    if kind == 'labels':
        return score, None, labels
    if kind == 'onehot':
        return score, F.one_hot(labels, K).float(), None
    if kind == 'acm':
        bg = torch.randint(-1, K, (B,), generator=g)
        return score, acm_targets(labels, bg, torch.rand(B, generator=g), 4.0, K), None
    soft = torch.softmax(torch.randn(B, K, generator=g), dim=1)
    return score, (soft if kind == 'softmax' else soft * 0.7), None


@functools.lru_cache(maxsize=None)
def softce_case(bi, kind, scale):
    score, soft, labels = softce_input(bi, kind, scale)
    r64 = soft_ce(score.double(), None if soft is None else soft.double(), labels)
    r32 = soft_ce(score, soft, labels)
    bars = dict(loss=bar(r64['loss'], r32['loss'], FLOOR_FN, CAP_FWD), dscore=bar(r64['dscore'], r32['dscore'], FLOOR_FN, CAP_GRAD5))
    return (score, soft, labels), r64, bars


# ---- feature-KD MSE ------------------------------------------------------------------------------------------------------

KD_NUMELS = [4, 1020, 1024, 4 * 262144 + 4, 4 * (2 * 262144 + 3)]    # one float4; off and on a block; one past, and two passes past,
KD_FWD_REL = 32 * U                                                    # ... the 4 * 256 * 1024 elements of a single grid pass
# forward: non-negative terms; each thread sums at most 3 trips of 4 squares, then a 6-level wave tree, 4 waves, an fp64 finalize.
KD_BWD_REL = 5 * U
# backward: c = fl(fl(fl(2 gh) / numel) * gdev), then fl(c * fl(a - b)): four roundings per element, no sum (5 U leaves one to spare)


def kd_mse(a, b):
    return ((a - b) ** 2).mean()


def kd_mse_grad(a, b, gscale_dev=1.0, gscale_host=1.0):
    return (a - b) * (2.0 * f32(gscale_host) * f32(gscale_dev) / a.numel())


def bf16_half_ulp(ref64):
    """Half a bf16 ulp (8 significand bits) at each value of ``ref64``: 2^(e - 9) for |v| = m 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(ref64)
    return torch.ldexp(torch.ones_like(ref64), e - 9)


def kd_input(numel, bf16=False):
    g = torch.Generator().manual_seed(22000 + numel % 9973)
    a, b = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
    return (a.bfloat16(), b.bfloat16()) if bf16 else (a, b)


# ---- optimizer -----------------------------------------------------------------------------------------------------------

SGD_NUMELS = [1, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 17]       # a tensor is walked in 32 chunks of 256: 8192 per pass
SQNORM_CAP = (1e-5, 0.0)


def sqnorm(tensors):
    """Sum of squares over all tensors, in their dtype (a python float)."""
    return float(sum((t * t).sum() for t in tensors))


def sqnorm_bar(tensors32):
    s64, s32 = sqnorm([t.double() for t in tensors32]), sqnorm(tensors32)
    return s64, bar(torch.tensor(s64), torch.tensor(s32, dtype=torch.float64), FLOOR_SUM, SQNORM_CAP)


def clip_coef(sq, grad_scale, max_norm):
    """min(max_norm / (sqrt(sq) * gs + 1e-6), 1); 1 when max_norm <= 0 (torch.nn.utils.clip_grad_norm_ on gradients scaled by gs)."""
    if max_norm <= 0:
        return 1.0
    return min(f32(max_norm) / (math.sqrt(sq) * f32(grad_scale) + f32(1e-6)), 1.0)


def sgd_step(p, g, buf, lr, wd, momentum, grad_scale=1.0, coef=1.0):
    """One SGD(momentum, weight decay) step in the dtype of ``p``: g' = g * gs * coef + wd * p, b' = m * b + g', p' = p - lr * b'.
    Returns (p', b', bar_p, bar_b): per element, 4u (|g gs coef| + |wd p| + |m b|) on the buffer and |lr| times that plus
    2u (|p| + |lr b'|) on the parameter -- the five roundings of an fp32 update and three more for gs * coef and the products."""
    lr, wd, m, gs = f32(lr), f32(wd), f32(momentum), f32(grad_scale)
    t_g, t_wd, t_mb = g * (gs * coef), wd * p, m * buf
    b2 = t_mb + (t_g + t_wd)
    p2 = p - lr * b2
    bar_b = 4 * U * (t_g.abs() + t_wd.abs() + t_mb.abs())
    bar_p = abs(lr) * bar_b + 2 * U * (p.abs() + (lr * b2).abs())
    return p2, b2, bar_p.double(), bar_b.double()
