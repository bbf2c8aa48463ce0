"""Plain-torch formulas of the time-channel importance distillation (csrc/tc_kd.hip, config key ``kd_importance``), computing
in the dtype of their inputs: run on fp64 tensors they are the reference the kernels are held against, run on fp32 tensors they
measure what fp32 itself loses.  Hooked outputs are logical (N, C, H, W), (N, D, 1, 1) or (N, D) with rows n = b * T + t; the map is
(T, C)."""
import torch

U = 2.0 ** -24          # fp32 unit roundoff

# (N, T, C, H, W); H = W = None: an (N, D) tensor
CASES = [(4, 2, 4, 1, 1), (6, 3, 8, None, None), (6, 3, 8, 5, 3), (16, 8, 68, 7, 7), (32, 8, 256, 14, 14)]
BF16_CASES = CASES[2:]


def case_shape(case):
    N, T, C, H, W = case
    return (N, C) if H is None else (N, C, H, W)


def make_case(case, seed=0, bf16=False, dtype=torch.float64):
    """(cur, prev, A): cur = relu(randn), prev = relu(cur + 0.3 randn) (stage outputs are relu outputs), A = rand + 0.1 renormalised
    to mean 1 in fp32 (the map's own type).  ``bf16``: cur and prev are rounded to bf16 first and then exact in ``dtype``."""
    N, T, C, H, W = case
    g = torch.Generator().manual_seed(1000 + seed)
    shape = case_shape(case)
    cur = torch.relu(torch.randn(shape, generator=g))
    prev = torch.relu(cur + 0.3 * torch.randn(shape, generator=g))
    if bf16:
        cur, prev = cur.bfloat16().float(), prev.bfloat16().float()
    A = torch.rand((T, C), generator=g) + 0.1
    A = (A / A.mean()).float()
    return cur.to(dtype), prev.to(dtype), A


def expand_map(A, like):
    """The (T, C) map as a tensor that broadcasts over ``like``: entry [n, c, ...] = A[n mod T, c]."""
    T, C = A.shape
    N = like.shape[0]
    assert N % T == 0 and like.shape[1] == C
    rows = A.to(like.dtype)[torch.arange(N) % T]                       # (N, C)
    return rows.reshape((N, C) + (1,) * (like.dim() - 2))


def weighted_loss(cur, prev, A):
    """L = 1 / numel * sum A[n mod T, c] * (cur - prev)^2"""
    d = cur - prev
    return (expand_map(A, cur) * d * d).sum() / cur.numel()


def weighted_grad(cur, prev, A, g=1.0):
    """dcur = g * 2 / numel * A[n mod T, c] * (cur - prev)"""
    return g * 2.0 / cur.numel() * expand_map(A, cur) * (cur - prev)


def sqgrad_sum(grad, T, scale=1.0):
    """S[t, c] = scale^2 * sum_{b,h,w} grad[b*T+t, c, h, w]^2"""
    N, C = grad.shape[0], grad.shape[1]
    g = grad.reshape(N // T, T, C, -1)
    return (scale * scale) * (g * g).sum(dim=(0, 3))


def normalise(S, count):
    """(A^, degenerate): raw = S / count, A^ = raw / mean(raw); all ones when mean(raw) is 0 or not finite."""
    raw = S / count if count else torch.full_like(S, float('nan'))
    m = raw.mean()
    if not torch.isfinite(m) or m <= 0:
        return torch.ones_like(raw), True
    return raw / m, False


def update(S, count, prev, task, mix=0.0):
    """(A_k, mixed): A_k = (k A_{k-1} + A^) / (k + 1) with A_0 = A^; mixed = (1 - mix) A_k + mix."""
    new, _ = normalise(S, count)
    if task > 0:
        new = (task * prev.to(new.dtype) + new) / (task + 1)
    return new, (1.0 - mix) * new + mix

