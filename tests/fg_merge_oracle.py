"""Torch restatement of the foreground-merging chain (csrc/fg_merge.hip; FAME-style, parity unpinned), stage by stage
and parameterised on ``dtype``: in torch.float32 every operation is the kernels' (same order of sums, every product and sum rounded
on its own); in torch.float64 it is the reference the GPU tests are held against.  Clips are planar (B, T, 3, H, W) here; ``to_nhwc4``
/ ``to_cthw`` make the other layouts.  Integer stages (bin indices, histograms, selection) are exact in either dtype."""
import torch

IMG_MEAN = (123.675, 116.28, 103.53)
IMG_STD = (58.395, 57.12, 57.375)


def tap_count(H, W):
    return 2 * (int(0.1 * min(H, W)) // 2) + 1


def blur_taps(H, W):
    """fp32 taps of the separable Gaussian: sigma = k / 3, computed and normalised in fp64."""
    k = tap_count(H, W)
    sigma = k / 3.0
    w = torch.tensor([(-((j - k // 2) ** 2) / (2 * sigma * sigma)) for j in range(k)], dtype=torch.float64).exp()
    return (w / w.sum()).float()


def colour_params(bins=8, mean=IMG_MEAN, std=IMG_STD):
    mean, std = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
    return (-mean / std).float(), (bins * std / 256).float()


def motion(x, dtype=torch.float64):
    """Stage 1: one accumulator per pixel, t outer, c inner."""
    x = x.to(dtype)
    B, T = x.shape[:2]
    acc = torch.zeros((B,) + tuple(x.shape[-2:]), dtype=dtype)
    for t in range(T - 1):
        for c in range(3):
            acc = acc + (x[:, t + 1, c] - x[:, t, c]).abs()
    return acc / torch.tensor(T - 1, dtype=dtype)


def _blur_last(m, taps, dtype):
    k = taps.numel()
    r = k // 2
    n = m.shape[-1]
    pad = torch.nn.functional.pad(m, (r, r), mode='reflect') if r else m      # (B, H, W): pads the last dimension, edge not repeated
    acc = torch.zeros_like(m)
    for j in range(k):
        acc = acc + taps[j].to(dtype) * pad[..., j:j + n]
    return acc


def blur(d, dtype=torch.float64):
    """Stage 2: along W, then along H; reflect border, taps in ascending order."""
    taps = blur_taps(*d.shape[-2:])
    d = d.to(dtype)
    a = _blur_last(d, taps, dtype)
    return _blur_last(a.transpose(-1, -2), taps, dtype).transpose(-1, -2).contiguous()


def quantise(g):
    """Stage 3 in g's dtype -> uint8 (B, H, W)."""
    lo = g.amin(dim=(-1, -2), keepdim=True)
    hi = g.amax(dim=(-1, -2), keepdim=True)
    m = (g - lo) / ((hi - lo) + torch.tensor(1e-8, dtype=g.dtype))
    q = torch.floor(torch.tensor(255.0, dtype=g.dtype) * m + torch.tensor(0.5, dtype=g.dtype))
    q = torch.where(hi == lo, torch.zeros_like(q), q)
    return q.clamp(0, 255).to(torch.uint8)


def motion_q(x, dtype=torch.float64):
    d = motion(x, dtype)
    g = blur(d, dtype)
    return quantise(g), g, d


def bin_index(x, bins=8, lo=None, scale=None):
    """Stage 4's bin index (B, T, H, W) int64, in x's dtype with the six fp32 constants widened; a NaN falls into bin 0."""
    if lo is None:
        lo, scale = colour_params(bins)
    v = torch.floor((x - lo.to(x.dtype).view(1, 1, 3, 1, 1)) * scale.to(x.dtype).view(1, 1, 3, 1, 1))
    v = torch.nan_to_num(v, nan=0.0, posinf=float(bins - 1), neginf=0.0).clamp(0, bins - 1).long()
    return (v[:, :, 0] * bins + v[:, :, 1]) * bins + v[:, :, 2]


def histograms(idx, q, bins=8):
    """F[b, i] = sum of q over the (t, h, w) in bin i, N[b, i] their count: int64 (B, bins^3)."""
    B, T = idx.shape[:2]
    nb = bins ** 3
    qq = q.long().unsqueeze(1).expand(B, T, *q.shape[-2:]).reshape(B, -1)
    flat = idx.reshape(B, -1)
    F = torch.zeros((B, nb), dtype=torch.int64).scatter_add_(1, flat, qq)
    N = torch.zeros((B, nb), dtype=torch.int64).scatter_add_(1, flat, torch.ones_like(qq))
    return F, N


def refine(idx, F, N, dtype=torch.float64):
    """Stage 5: s = (sum over t ascending of F[i_t] / (255 * N[i_t])) / T."""
    B, T = idx.shape[:2]
    ratio = torch.where(N > 0, F.to(dtype) / (torch.tensor(255.0, dtype=dtype) * N.clamp(min=1).to(dtype)), torch.zeros((), dtype=dtype))
    acc = torch.zeros((B,) + tuple(idx.shape[-2:]), dtype=dtype)
    for t in range(T):
        acc = acc + torch.gather(ratio, 1, idx[:, t].reshape(B, -1)).view_as(acc)
    return acc / torch.tensor(T, dtype=dtype)


def k_fg(beta, H, W):
    return max(1, int(beta * H * W))


def select(s, k):
    """Stage 6: v = k-th largest of s[b]; foreground = (s >= v and s > 0).  -> (v (B,), mask uint8 like s, count int64 (B,))."""
    B = s.shape[0]
    v = torch.topk(s.reshape(B, -1), k, dim=1).values[:, -1]
    mask = (s >= v.view((B,) + (1,) * (s.dim() - 1))) & (s > 0)
    return v, mask.to(torch.uint8), mask.reshape(B, -1).sum(1)


def foreground_mask(x, beta=0.5, bins=8, mean=IMG_MEAN, std=IMG_STD, dtype=torch.float64):
    """The whole chain on a planar clip batch -> (s, mask uint8 (B, H, W), count, q)."""
    lo, scale = colour_params(bins, mean, std)
    q, _, _ = motion_q(x, dtype)
    idx = bin_index(x.float(), bins, lo, scale)      # the bins are DEFINED on the fp32 clip: an 8-bit pixel value sits exactly on an edge
    F, N = histograms(idx, q, bins)
    s = refine(idx, F, N, dtype)
    _, mask, count = select(s, k_fg(beta, *x.shape[-2:]))
    return s, mask, count, q


def merge(x, mask, count, perm, apply):
    """Stage 7 on a planar (B, T, 3, H, W) batch, out of place: gather, then assign."""
    before = x.clone()
    out = x.clone()
    for b in range(x.shape[0]):
        p = int(perm[b])
        if bool(apply[b]) and p != b and int(count[b]) > 0:
            out[b] = torch.where(mask[b].bool().view(1, 1, *mask.shape[-2:]), before[b], before[p])
    return out


# ---- layouts and scenes ------------------------------------------------------------------------------------------------------------

def to_nhwc4(x, lane=None):
    """(B, T, 3, H, W) -> (B*T, H, W, 4); the fourth lane holds ``lane`` (default: a pattern that names clip and pixel)."""
    B, T, _, H, W = x.shape
    out = torch.empty((B * T, H, W, 4), dtype=x.dtype)
    out[..., :3] = x.reshape(B * T, 3, H, W).permute(0, 2, 3, 1)
    out[..., 3] = (torch.arange(B * T * H * W, dtype=x.dtype).view(B * T, H, W) % 251) + 1000 if lane is None else lane
    return out


def from_nhwc4(y, B, T):
    return y[..., :3].permute(0, 3, 1, 2).reshape(B, T, 3, *y.shape[1:3]).contiguous()


def to_cthw(x):
    """(B, T, 3, H, W) -> (B, 1, 3, T, H, W), the 3-D recognizer's batch with one clip."""
    return x.permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()


def normalise(raw, mean=IMG_MEAN, std=IMG_STD):
    m = torch.tensor(mean, dtype=torch.float32).view(1, 1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 1, 3, 1, 1)
    return ((raw.float() - m) / s).contiguous()


def two_halves_scene(B, T, H, W, seed=0):
    """Left half of every frame: fresh noise with R in 160..250, B in 0..60; right half static with R in 0..60, B in 160..250; G free.
    -> normalised fp32 (B, T, 3, H, W).  The left half is columns [0, W // 2)."""
    g = torch.Generator().manual_seed(seed)
    half = W // 2
    raw = torch.empty((B, T, 3, H, W), dtype=torch.float32)
    raw[:, :, 0, :, :half] = torch.randint(160, 251, (B, T, H, half), generator=g).float()
    raw[:, :, 1, :, :half] = torch.randint(0, 256, (B, T, H, half), generator=g).float()
    raw[:, :, 2, :, :half] = torch.randint(0, 61, (B, T, H, half), generator=g).float()
    raw[:, :, 0, :, half:] = torch.randint(0, 61, (B, 1, H, W - half), generator=g).float()
    raw[:, :, 1, :, half:] = torch.randint(0, 256, (B, 1, H, W - half), generator=g).float()
    raw[:, :, 2, :, half:] = torch.randint(160, 251, (B, 1, H, W - half), generator=g).float()
    return normalise(raw)


def random_clip(B, T, H, W, seed=0):
    """A normalised clip of smooth moving content plus noise: a motion map with structure at every scale."""
    g = torch.Generator().manual_seed(1000 + seed)
    raw = torch.randint(0, 256, (B, 1, 3, H, W), generator=g).float().repeat(1, T, 1, 1, 1)
    yy = torch.arange(H).view(H, 1).float()
    xx = torch.arange(W).view(1, W).float()
    for b in range(B):
        for t in range(T):
            blob = torch.exp(-((yy - H * (0.3 + 0.1 * t)) ** 2 + (xx - W * (0.2 + 0.15 * b + 0.05 * t)) ** 2) / (0.02 * H * W + 1))
            raw[b, t] = raw[b, t] * (1 - blob) + blob * torch.randint(0, 256, (3, H, W), generator=g).float()
    return normalise(raw.round())
