"""Reference side of the pooled-output distillation tests (tests/test_pod_kd_cpu.py, tests/test_pod_kd_gpu.py).

UPSTREAM, unpinned: the two formulas restate PODNet's ``pod(collapse_channels='spatial', normalize=True)`` and
``embeddings_similarity`` (Douillard et al., ECCV 2020) from the paper; the reference repository has no such loss, so there is no
golden vector.  Everything here is plain torch on the CPU and computes in the dtype of its inputs (fp64 is the reference the
kernels are held against, fp32 gives the deviation term of the bars).

  * ``pod_spatial`` / ``pod_flat``: the formulas, differentiated by autograd;
  * ``pod_spatial_closed`` / ``pod_flat_closed``: the closed-form gradients csrc/pod_kd.hip implements;
  * the case tables and seeded inputs; the summation depths of the kernels and the bars built from them.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-12
U = 2.0 ** -24          # fp32 unit roundoff

# (N, C, H, W); the last one sits at the kernels' H / W limit
MAX_HW = 64
SPATIAL_CASES = [(1, 4, 1, 1), (3, 4, 5, 3), (3, 68, 7, 7), (2, 8, 56, 56), (2, 2048, 7, 7), (5, 64, 1, 9), (2, 4, MAX_HW, MAX_HW)]
FLAT_CASES = [(1, 4), (3, 68), (5, 2048), (130, 512)]
# CPU-only closed-form cases: name -> what is special about the inputs
SPECIAL = ('cur_eq_prev', 'zero_cur_frame', 'zero_prev_frame')


def pod_spatial(cur, prev):
    """cur, prev: logical (N, C, H, W).  mean_n | normalize(concat(sum_w cur^2, sum_h cur^2)) - the same of prev |."""
    a, b = cur.pow(2), prev.pow(2)
    p = torch.cat([a.sum(3).flatten(1), a.sum(2).flatten(1)], dim=1)
    q = torch.cat([b.sum(3).flatten(1), b.sum(2).flatten(1)], dim=1)
    p, q = F.normalize(p, dim=1, p=2, eps=EPS), F.normalize(q, dim=1, p=2, eps=EPS)
    return torch.linalg.vector_norm(p - q, dim=1).mean()


def pod_flat(cur, prev):
    """cur, prev: (N, D) or (N, D, 1, 1)."""
    c, p = cur.flatten(1), prev.flatten(1)
    return F.cosine_embedding_loss(c, p, torch.ones(c.shape[0], dtype=c.dtype))


def profiles(x):
    """(N, C, H, W) -> (N, H+W, C): the layout of the kernels' profile and G tensors."""
    a = x.pow(2)
    return torch.cat([a.sum(3).permute(0, 2, 1), a.sum(2).permute(0, 2, 1)], dim=1)


def pod_spatial_closed(cur, prev):
    """(loss, G, dcur, dist): G (N, H+W, C) = d loss / d profile, dcur = 2 cur (G[n,h,c] + G[n,H+w,c]), dist (N,) per frame."""
    N, C, H, W = cur.shape
    P, Q = profiles(cur), profiles(prev)
    np_, nq = P.flatten(1).norm(dim=1), Q.flatten(1).norm(dim=1)
    ph, qh = P / np_.clamp_min(EPS)[:, None, None], Q / nq.clamp_min(EPS)[:, None, None]
    d = ph - qh
    dist = d.flatten(1).norm(dim=1)
    nz = dist > 0
    u = torch.where(nz[:, None, None], d / torch.where(nz, dist, torch.ones_like(dist))[:, None, None], torch.zeros_like(d))
    pu = (ph * u).flatten(1).sum(1)
    m = (np_ >= EPS).to(cur.dtype)                      # clamp_min's backward inside F.normalize
    G = (u - (m * pu)[:, None, None] * ph) / np_.clamp_min(EPS)[:, None, None] / N
    gh, gw = G[:, :H].permute(0, 2, 1), G[:, H:].permute(0, 2, 1)       # (N, C, H), (N, C, W)
    dcur = 2 * cur * (gh[:, :, :, None] + gw[:, :, None, :])
    return dist.mean(), G, dcur, dist


def pod_flat_closed(cur, prev):
    """(loss, dcur) with dcur in cur's shape."""
    c, p = cur.flatten(1), prev.flatten(1)
    N = c.shape[0]
    dot, mc, mp = (c * p).sum(1), (c * c).sum(1) + EPS, (p * p).sum(1) + EPS
    den = (mc * mp).sqrt()
    loss = (1 - dot / den).mean()
    dcur = -(p - c * (dot / mc)[:, None]) / den[:, None] / N
    return loss, dcur.reshape(cur.shape)


def make_case(shape, seed=0, bf16=False, dtype=torch.float64):
    """cur = relu(randn), prev = relu(cur + 0.3 randn), drawn in fp32 on the CPU; bf16: rounded to bf16 first (then exact in fp64)."""
    g = torch.Generator().manual_seed(1000 + seed)
    cur = torch.relu(torch.randn(*shape, generator=g))
    prev = torch.relu(cur + 0.3 * torch.randn(*shape, generator=g))
    if bf16:
        cur, prev = cur.bfloat16().float(), prev.bfloat16().float()
    return cur.to(dtype), prev.to(dtype)


def special_case(kind, shape=(3, 8, 5, 6), dtype=torch.float64):
    cur, prev = make_case(shape, seed=77, dtype=dtype)
    if kind == 'cur_eq_prev':
        prev = cur.clone()
    elif kind == 'zero_cur_frame':
        cur[1] = 0
    elif kind == 'zero_prev_frame':
        prev[1] = 0
    else:
        raise KeyError(kind)
    return cur, prev


# ---- summation depths of csrc/pod_kd.hip and the bars ------------------------------------------------------------------------

def spatial_depth(C, H, W):
    """Roundings that reach one normalised profile entry.  A row sum: 1 (square) + ceil(W/4) terms per thread + 2 shuffle levels;
    a column sum: 1 + ceil(H/4) terms per thread + 3 adds across the waves.  The squared norm adds, per thread, 4 components of at
    most ceil(H/4) + ceil(W/4) entries, a 6-level wave tree and 2 levels across waves (slabs are summed in fp64); the square root
    halves its share, the entries' own error enters the norm once.  2 more for the reciprocal and the product."""
    prof = max(1 + math.ceil(W / 4) + 2, 1 + math.ceil(H / 4) + 3)
    norm = prof + (4 * (math.ceil(H / 4) + math.ceil(W / 4)) + 6 + 2 + 1) / 2
    return prof + norm + 2


def frame_sum_depth(C, H, W):
    """pod_frame_kernel's two sums: 4 components of ceil((H+W) C / 4 / 256) float4 per thread, 6 wave levels, 2 across waves."""
    return 4 * math.ceil((H + W) * C / 4 / 256) + 6 + 2


def spatial_loss_floor(C, H, W):
    """Absolute: |d p^| + |d q^| <= depth * U * (|p^| + |q^|) = 2 depth U moves a distance by as much; the sum of squares and the
    square root add (frame_sum_depth / 2 + 1) U relative to a distance of at most 2."""
    return (2 * spatial_depth(C, H, W) + 2 * (frame_sum_depth(C, H, W) / 2 + 1)) * U


def spatial_grad_floor(C, H, W, dist_min, scale):
    """Relative to ``scale`` = max |dcur|: the unit vector u = d / dist carries 2 depth U / dist from d and again as much from
    dist; p^.u the same plus its own sum; 6 for the products up to dcur."""
    return (4 * spatial_depth(C, H, W) / dist_min + frame_sum_depth(C, H, W) + 6) * U * scale


def flat_depth(D):
    """One of pod_flat_kernel's three sums: 4 components of ceil(D / 256) float4 per lane, 6 wave levels."""
    return 4 * math.ceil(D / 256) + 6


def flat_loss_floor(D):
    """cos = dot / sqrt(mc mp) <= 1 with non-negative terms everywhere (inputs are relu outputs): dot, and half of mc and mp."""
    return (2 * flat_depth(D) + 4) * U


def flat_grad_floor(cur64, prev64):
    """dcur = k (prev - cur r): r = dot / mc and k = -1 / (N den) carry (2 flat_depth + 4) U relative, and they act on the two terms
    before these cancel: (2 flat_depth + 8) U * max |k| (|prev| + |cur| r)."""
    c, p = cur64.flatten(1), prev64.flatten(1)
    dot, mc, mp = (c * p).sum(1), (c * c).sum(1) + EPS, (p * p).sum(1) + EPS
    k = 1 / (mc * mp).sqrt() / c.shape[0]
    amp = (k[:, None] * (p.abs() + c.abs() * (dot / mc).abs()[:, None])).max().item()
    return (2 * flat_depth(c.shape[1]) + 8) * U * amp


def bar(floor, dev32, cap):
    """floor + 4 x (fp32 CPU run - fp64 run), never looser than the project's cap for the quantity."""
    return min(floor + 4 * dev32, cap)


def loss_cap(ref):
    return 1e-5 * abs(float(ref)) + 1e-6


def grad_cap(ref):
    return 1e-4 * ref.abs().max().item() + 1e-7


def bf16_half_ulp(ref64):
    """Half a bf16 ulp of each value (0 at 0): 2^(e - 9) for |v| = m 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(ref64)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), torch.ldexp(torch.ones_like(ref64), e - 9))
