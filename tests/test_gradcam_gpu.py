"""csrc/gradcam.hip and ``bdvcil_amd.GradCAM`` on the GPU.

Kernel level: every output against an fp64 numpy / torch-CPU restatement written here, with bounds derived where they are applied
(u = one ulp of fp32 = 2^-24 relative):
  * map: a lane adds its products with fmaf (one rounding each), a fixed tree adds the lanes: at most C + 4 roundings on the way, each
    at most u times the running sum of magnitudes -> (C + 4) * u * sum_c |wgt * A| per pixel; dyadic inputs are exact in any order;
  * upsampled map: two taps a, b per axis as a + l (b - a) with the coordinate in fp64: rounding of l, of b - a, of the product, of
    the sum = under 4 u max|m| per axis, 8 u max|m| for both;
  * v = (u - min) / ((max - min) + 1e-20f): IEEE operations on the kernel's own u, reproduced exactly in numpy float32;
  * overlay: a handful of fp32 roundings on values in [0, 1], scaled by 255, then rint: 0.5 + 255 * 8 u;
  * box sums: fp64 accumulation in a fixed order, one rounding to fp32 each: 2 u relative.
The kernel's own u is read back without a further kernel by rendering with (min, max) = (0, 1): v = (u - 0) / (1 + 1e-20f) = u.

Model level: the CPU oracle model (oracle.tsm_oracle, imported, not modified) with a plain forward hook and ``retain_grad``, in fp32
and, converted with ``.double()``, in fp64.  The map's bar is not invented: d0 = max |map(fp32 oracle) - map(fp64 oracle)| on the
test's own inputs, and the GPU map must lie within 4 * d0 of the fp64 one (the GPU differs from fp64 as the fp32 CPU does, by the
summation order inside each convolution, through about twice as many reorderings).  Seeds are fixed to ones where d0 <= 1e-3 (checked).
Measured (profiles/gradcam.txt): see the table beside ``MODEL_CASES``."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pool_oracle as P
from oracle import tsm_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _k():
    from bdvcil_amd import kernels as K
    return K


def _poison(dev, *tensors_like):
    """Best effort, as tests/test_pool_kernels_gpu.py: fill and free blocks of the outputs' sizes with 0xFF (NaN / 255) right before
    the call, which the caching allocator usually hands to the wrapper next."""
    blocks = [torch.full((int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev)
              for shape, dtype in tensors_like]
    torch.cuda.synchronize()
    del blocks


# ---- bdv_gradcam_map -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [4, 64, 68, 512, 2048])
def test_map_against_fp64(C, dev):
    K = _k()
    for (h, w) in ((1, 1), (2, 2), (7, 7), (5, 3)):
        for N in (1, 5, 16):
            seed = 1000 * C + 10 * h * w + N
            rng = np.random.default_rng(seed)
            cases = {'dyadic': (P.dyadic((N, h, w, C), seed), P.dyadic((N, C), seed + 1)),
                     'randn': (rng.standard_normal((N, h, w, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)),
                     'all products negative': (np.abs(P.dyadic((N, h, w, C), seed + 2)) + 0.125, -np.abs(P.dyadic((N, C), seed + 3)) - 0.125)}
            for name, (A, wgt) in cases.items():
                A, wgt = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(wgt, dtype=np.float32)
                prod = A.astype(np.float64) * wgt.astype(np.float64)[:, None, None, :]
                ref = np.maximum(prod.sum(-1), 0.0)
                Ad, wd = torch.from_numpy(A).to(dev), torch.from_numpy(wgt).to(dev)
                _poison(dev, ((N, h, w), torch.float32))
                got = K.gradcam_map(Ad, wd).cpu().numpy()
                what = f'{name} N={N} {h}x{w} C={C}'
                assert got.shape == (N, h, w) and got.dtype == np.float32, what
                if name == 'randn':
                    bound = (C + 4) * U * np.abs(prod).sum(-1)
                    err = np.abs(got.astype(np.float64) - ref)
                    assert (err <= bound).all(), f'{what}: err {err.max():.3e}, worst err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}'
                else:
                    assert np.array_equal(got, ref.astype(np.float32)), what
                if name == 'all products negative':
                    assert not got.any() and not np.signbit(got).any(), what


def test_map_argument_checks(dev):
    K = _k()
    A = torch.zeros(2, 3, 3, 8, device=dev)
    with pytest.raises(ValueError):
        K.gradcam_map(torch.zeros(2, 3, 3, 6, device=dev), torch.zeros(2, 6, device=dev))       # C % 4
    with pytest.raises(ValueError):
        K.gradcam_map(A, torch.zeros(3, 8, device=dev))
    with pytest.raises(ValueError):
        K.gradcam_map(A.permute(0, 3, 1, 2), torch.zeros(2, 3, device=dev))                      # not contiguous
    with pytest.raises(TypeError):
        K.gradcam_map(A.half(), torch.zeros(2, 8, device=dev))
    with pytest.raises(TypeError):
        K.gradcam_map(A.cpu().numpy(), torch.zeros(2, 8, device=dev))


# ---- bdv_gradcam_minmax / bdv_gradcam_render: the map output ----------------------------------------------------------------------

UP_CASES = [((1, 1), (8, 8), B, T) for B in (1, 3) for T in (1, 8)] + [((2, 2), (64, 64), B, T) for B in (1, 3) for T in (1, 8)] + \
    [((7, 7), (224, 224), 1, 2)] + [((3, 5), (17, 23), B, T) for B in (1, 3) for T in (1, 8)] + [((4, 4), (4, 4), B, T) for B in (1, 3) for T in (1, 8)]


def _clip_maps(B, T, h, w, seed):
    """Non-negative maps with exact zeros (a ReLU output).  T = 8: clip 0's maximum lies in frame 0 and its minimum in the last frame;
    B = 3: clip 1 is all zero and clip 2 a constant that is no power of two."""
    rng = np.random.default_rng(seed)
    m = np.maximum(rng.standard_normal((B, T, h, w)), 0.0).astype(np.float32)
    if T == 8:
        m[0, :-1] += 1.0
        m[0, 0, 0, 0] = 9.5
        m[0, -1] = 0.25 * m[0, -1] + 0.03125
    if B == 3:
        m[1] = 0.0
        m[2] = np.float32(0.7)
    return m


def _kernel_u(K, md, B, T, H, W, dev):
    unit = torch.tensor([[0.0] * B, [1.0] * B], device=dev)
    return K.gradcam_render(md, unit, B, T, H, W)[0]


@pytest.mark.parametrize('hw,HW,B,T', UP_CASES)
def test_upsample_minmax_and_normalised_map(hw, HW, B, T, dev):
    K = _k()
    (h, w), (H, W) = hw, HW
    m = _clip_maps(B, T, h, w, 7 * h + w + 100 * B + T)
    md = torch.from_numpy(m).reshape(B * T, h, w).to(dev)
    ref = F.interpolate(torch.from_numpy(m).double().reshape(B * T, 1, h, w), size=(H, W), mode='bilinear', align_corners=False)
    ref = ref.reshape(B, T, H, W).numpy()
    _poison(dev, ((B, T, H, W), torch.float32))
    u = _kernel_u(K, md, B, T, H, W, dev).cpu().numpy()
    err = np.abs(u.astype(np.float64) - ref).max()
    print(f'{hw}->{HW} B={B} T={T}: upsample err {err:.3e}, bound {8 * U * m.max():.3e}')
    assert err <= 8 * U * max(float(m.max()), 0.0)
    if (h, w) == (H, W):
        assert np.array_equal(u, m)
    _poison(dev, ((2, B), torch.float32))
    mm = K.gradcam_minmax(md, B, T, H, W)
    mmh = mm.cpu().numpy()
    flat = u.reshape(B, -1)
    assert np.array_equal(mmh[0], flat.min(1)) and np.array_equal(mmh[1], flat.max(1)), (mmh, flat.min(1), flat.max(1))
    _poison(dev, ((B, T, H, W), torch.float32))
    v = K.gradcam_render(md, mm, B, T, H, W)[0].cpu().numpy()
    assert np.isfinite(v).all()
    mn, mx = mmh[0][:, None, None, None], mmh[1][:, None, None, None]
    want = (u - mn) / ((mx - mn) + np.float32(1e-20))                       # float32 throughout, IEEE division on both sides
    assert want.dtype == np.float32 and np.array_equal(v, want)
    for b in range(B):
        top = (mmh[1, b] - mmh[0, b]) / ((mmh[1, b] - mmh[0, b]) + np.float32(1e-20))
        assert v[b].min() == 0.0 and v[b].max() == top, (b, v[b].min(), v[b].max(), top)
    if T == 8:
        fmax, fmin = np.unravel_index(u[0].argmax(), u[0].shape)[0], np.unravel_index(u[0].argmin(), u[0].shape)[0]
        assert fmax == 0 and fmin == T - 1                                  # the extremes lie in different frames: one scale per clip
    if B == 3:
        assert not v[1].any() and not v[2].any()                            # all-zero clip, constant clip: zeros, never NaN
        assert mmh[0, 2] == mmh[1, 2] == np.float32(0.7)


def test_minmax_and_render_argument_checks(dev):
    K = _k()
    m = torch.zeros(4, 2, 2, device=dev)
    mm = torch.zeros(2, 2, device=dev)
    with pytest.raises(ValueError):
        K.gradcam_minmax(m, 3, 2, 8, 8)
    with pytest.raises(ValueError):
        K.gradcam_minmax(m, 2, 2, 0, 8)
    with pytest.raises(TypeError):
        K.gradcam_minmax(m.double(), 2, 2, 8, 8)
    with pytest.raises(ValueError):
        K.gradcam_render(m, torch.zeros(2, 3, device=dev), 2, 2, 8, 8)
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, want_map=False)                                                # nothing requested
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, frames4=torch.zeros(4, 8, 8, 4, device=dev))                  # no lut
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, frames4=torch.zeros(4, 8, 8, 4, device=dev), lut=torch.zeros(256, 3, device=dev), alpha=2.0,
                         mean=(0, 0, 0), std=(1, 1, 1))
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, frames4=torch.zeros(4, 8, 8, 4, device=dev), lut=torch.zeros(16, 3, device=dev),
                         mean=(0, 0, 0), std=(1, 1, 1))
    one = np.array([[0, 0, 4, 4]], np.float32)
    with pytest.raises(ValueError, match='decrease'):
        K.gradcam_render(m, mm, 2, 2, 8, 8, box_offsets=[0, 1, 0, 1, 1], boxes=one)                       # offsets not monotone
    with pytest.raises(ValueError, match='rows'):
        K.gradcam_render(m, mm, 2, 2, 8, 8, box_offsets=[0, 1, 1, 2, 2], boxes=one)                       # row count does not match
    with pytest.raises(ValueError, match='offsets'):
        K.gradcam_render(m, mm, 2, 2, 8, 8, box_offsets=[0, 1, 1], boxes=one)
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, box_offsets=[0, 1, 1, 1, 1], boxes=np.full((1, 4), np.nan, np.float32))
    with pytest.raises(ValueError):
        K.gradcam_render(m, mm, 2, 2, 8, 8, box_offsets=[0, 0, 0, 0, 0])


# ---- overlay ----------------------------------------------------------------------------------------------------------------------

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def _luts():
    out = [('random', np.random.default_rng(11).random((256, 3)).astype(np.float32))]
    try:
        import matplotlib
        out.append(('viridis', np.asarray(matplotlib.colormaps['viridis'](np.arange(256))[:, :3], dtype=np.float32)))
    except ImportError:         # matplotlib is optional: the random table is the case that always runs
        pass
    return out


@pytest.mark.parametrize('alpha', [0.0, 0.5, 1.0])
def test_overlay_against_fp64(alpha, dev):
    K = _k()
    B, T, h, w, H, W = 2, 2, 3, 5, 17, 23
    m = _clip_maps(B, T, h, w, 5)
    md = torch.from_numpy(m).reshape(B * T, h, w).to(dev)
    rng = np.random.default_rng(6)
    pix = rng.integers(0, 256, (B * T, H, W, 3)).astype(np.uint8)
    mean32, std32 = np.array(MEAN, np.float32), np.array(STD, np.float32)
    x = np.zeros((B * T, H, W, 4), np.float32)
    x[..., :3] = (pix.astype(np.float32) - mean32) / std32
    xd = torch.from_numpy(x).to(dev)
    mm = K.gradcam_minmax(md, B, T, H, W)
    mmh = mm.cpu().numpy().astype(np.float64)
    u64 = F.interpolate(torch.from_numpy(m).double().reshape(B * T, 1, h, w), size=(H, W), mode='bilinear', align_corners=False)
    u64 = u64.reshape(B, T, H, W).numpy()
    mn, mx = u64.reshape(B, -1).min(1)[:, None, None, None], u64.reshape(B, -1).max(1)[:, None, None, None]
    v64 = (u64 - mn) / (mx - mn + 1e-20)
    # how far the kernel's v may lie from v64: numerator and denominator each carry two upsampling errors of 8 u max|m|, plus the
    # roundings of the subtraction and the division
    eps = 2 * (2 * 8 * U * float(m.max())) / (mx - mn) + 4 * U
    img01 = (x[..., :3].astype(np.float64) * std32.astype(np.float64) + mean32.astype(np.float64)) / 255.0
    img01 = img01.reshape(B, T, H, W, 3)
    for name, lut in _luts():
        _poison(dev, ((B, T, H, W, 3), torch.uint8), ((B, T, H, W), torch.float32))
        v, ov, _ = K.gradcam_render(md, mm, B, T, H, W, True, xd, torch.from_numpy(lut).to(dev), alpha, MEAN, STD)
        ov = ov.cpu().numpy()
        assert ov.shape == (B, T, H, W, 3) and ov.dtype == np.uint8
        best = np.full(ov.shape, np.inf)
        for d in (-1.0, 0.0, 1.0):            # the fp64 index, or its neighbour where 256 * v64 lies within the map bound of an integer
            idx = np.clip(np.floor(256.0 * np.clip(v64 + d * eps, 0.0, None)), 0, 255).astype(np.int64)
            q = 255.0 * np.clip(alpha * lut.astype(np.float64)[idx] + (1.0 - alpha) * img01, 0.0, 1.0)
            best = np.minimum(best, np.abs(ov.astype(np.float64) - q))
        print(f'overlay {name} alpha={alpha}: worst distance to the un-rounded value {best.max():.6f} (bound {0.5 + 255 * 8 * U:.6f})')
        assert best.max() <= 0.5 + 255 * 8 * U
        if alpha == 0.0:
            assert np.array_equal(ov, pix.reshape(B, T, H, W, 3))                                   # the de-normalised frame
        if alpha == 1.0:
            own = np.minimum(255, np.floor(np.float32(256.0) * v.cpu().numpy())).astype(np.int64)   # the kernel's own index
            assert np.array_equal(ov, np.rint(np.float32(255.0) * lut[own]).astype(np.uint8))       # the table's colour


# ---- box sums ---------------------------------------------------------------------------------------------------------------------

def _inside(boxes, H, W):
    """Union of boxes rasterised on pixel centres, float32 comparisons as the kernel makes them."""
    cy, cx = np.arange(H, dtype=np.float32)[:, None] + np.float32(0.5), np.arange(W, dtype=np.float32)[None, :] + np.float32(0.5)
    mask = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in np.asarray(boxes, np.float32).reshape(-1, 4):
        mask |= (x0 <= cx) & (cx < x1) & (y0 <= cy) & (cy < y1)
    return mask


def test_box_sums(dev):
    from bdvcil_amd import gradcam as G
    K = _k()
    B, T, h, w, H, W = 4, 2, 3, 5, 17, 23
    m = _clip_maps(B, T, h, w, 9)
    m[3] = 0.0                                                                  # a clip with boxes and an empty map
    md = torch.from_numpy(m).reshape(B * T, h, w).to(dev)
    boxes = [[[[2.0, 3.0, 12.5, 9.0], [8.0, 5.5, 20.0, 14.0]],                  # two overlapping boxes: their union, no double count
              [[4.0, 4.0, 4.0, 12.0], [-6.0, -3.0, 5.5, 7.5], [18.5, 10.0, 40.0, 30.0]]],   # degenerate (x0 == x1); two partly outside
             [[[1.0, 1.0, 22.0, 16.0]], []],                                    # boxes in some frames only
             [[], []],                                                          # no box at all
             [[[0.0, 0.0, 23.0, 17.0]], []]]
    off, rows = G.box_table(boxes, B, T)
    mm = K.gradcam_minmax(md, B, T, H, W)
    _poison(dev, ((B, 2), torch.float32))
    v, _, sums = K.gradcam_render(md, mm, B, T, H, W, True, box_offsets=off, boxes=rows)
    again = K.gradcam_render(md, mm, B, T, H, W, False, box_offsets=off, boxes=rows)[2]
    assert torch.equal(sums, again)                                              # bit-identical from run to run
    v64 = v.cpu().numpy().astype(np.float64)
    mask = np.stack([np.stack([_inside(boxes[b][t], H, W) for t in range(T)]) for b in range(B)])
    assert mask[0, 0].sum() < _inside(boxes[0][0][:1], H, W).sum() + _inside(boxes[0][0][1:], H, W).sum()      # they do overlap
    assert mask[0, 1].sum() == _inside(boxes[0][1][1:], H, W).sum() > 0                                          # the degenerate box adds nothing
    want = np.stack([v64.reshape(B, -1).sum(1), (v64 * mask).reshape(B, -1).sum(1)], 1)
    got = sums.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 2 * U * want).all(), (got, want)
    has_box = torch.tensor([True, True, False, True])
    att = G.actor_attention_ratio(sums, has_box).cpu().numpy()
    assert np.isnan(att[2]) and np.isnan(att[3]) and 0.0 < att[0] < 1.0 and 0.0 < att[1] < 1.0
    assert abs(att[0] - want[0, 1] / want[0, 0]) <= 5 * U
    # one full-frame box in every frame: the two sums add the same values in the same order
    full = [[[[0.0, 0.0, float(W), float(H)]]] * T] * B
    s_full = K.gradcam_render(md, mm, B, T, H, W, False, box_offsets=G.box_table(full, B, T)[0], boxes=G.box_table(full, B, T)[1])[2].cpu().numpy()
    assert (np.abs(s_full[:3, 1] / s_full[:3, 0] - 1.0) <= 4 * U).all() and s_full[3, 0] == 0.0
    # no boxes anywhere: defined sums, undefined ratio
    none = K.gradcam_render(md, mm, B, T, H, W, False, box_offsets=np.zeros(B * T + 1, np.int64), boxes=np.zeros((0, 4), np.float32))[2]
    assert not none[:, 1].any() and torch.equal(none[:, 0], sums[:, 0])
    assert np.isnan(G.actor_attention_ratio(none, torch.zeros(B, dtype=torch.bool)).cpu().numpy()).all()


# ---- the model: bdvcil_amd.GradCAM against the CPU oracle -------------------------------------------------------------------------

K_CLASSES, B_, T_, S_ = 5, 2, 8, 64

# (depth, target layer, weight seed, input seed).  Measured (profiles/gradcam.txt): d0 on the CPU, then the GPU map's distance to
# the fp64 map on an MI355X under bf16x3 / f32mfma, in units of d0 -- the bar is 4 d0:
#   R18 layer4    d0 1.274e-06   1.67 / 1.43
#   R18 layer3    d0 1.471e-06   1.62 / 0.99
#   R18 layer4.1  d0 1.274e-06   1.67 / 1.43
#   R50 layer4    d0 1.985e-06   1.35 / 1.52
MODEL_CASES = [
    (18, 'backbone.layer4', 0, 1),
    (18, 'backbone.layer3', 0, 1),
    (18, 'backbone.layer4.1', 0, 1),
    (50, 'backbone.layer4', 0, 1),
]

_ORACLE = {}


def _rget(obj, path):
    for part in path.split('.'):
        obj = getattr(obj, part)
    return obj


def _inputs(depth, wseed, iseed):
    torch.manual_seed(wseed)
    cfg = O.r50_cfg(num_classes=K_CLASSES, depth=depth, head='LocalSimilarityClassifier', loss='LSCLoss', dropout_ratio=0.0)
    ref = O.build_model(copy.deepcopy(cfg))
    g = torch.Generator().manual_seed(iseed)
    imgs = torch.randn(B_, T_, 3, S_, S_, generator=g)
    labels = torch.randint(0, K_CLASSES, (B_,), generator=g)
    return cfg, ref, imgs, labels


def oracle_cam(ref, imgs, labels, layer):
    """mmaction2's GradCAM._calculate_localization_map on the oracle model: forward hook + retain_grad, zero_grad + backward, weights =
    spatial mean of the gradient, relu, bilinear upsampling, min-max per sample with delta 1e-20.  dtype follows ``imgs``."""
    ref.eval()
    ref.test_cfg['average_clips'] = 'score'
    feats = {}

    def hook(module, inputs, output):
        output.retain_grad()
        feats['a'] = output
    handle = _rget(ref, layer).register_forward_hook(hook)
    try:
        preds = ref(imgs, return_loss=False)
    finally:
        handle.remove()
    pick = preds.argmax(1) if labels is None else labels
    score = preds.gather(1, pick.view(-1, 1)).sum()
    ref.zero_grad()
    score.backward()
    A, G = feats['a'], feats['a'].grad
    wgt = G.mean(dim=(2, 3), keepdim=True)
    m = F.relu((wgt * A).sum(dim=1, keepdim=True))
    Bn, Tn, H, W = imgs.shape[0], imgs.shape[1], imgs.shape[3], imgs.shape[4]
    up = F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False).reshape(Bn, Tn, H, W)
    mn = up.reshape(Bn, -1).min(1).values.view(Bn, 1, 1, 1)
    mx = up.reshape(Bn, -1).max(1).values.view(Bn, 1, 1, 1)
    return ((up - mn) / (mx - mn + 1e-20)).detach(), preds.detach()


def _oracle(depth, layer, wseed, iseed, with_labels=True):
    """fp32 and fp64 oracle maps of one case, computed once and shared (never modified)."""
    key = (depth, layer, wseed, iseed, with_labels)
    if key not in _ORACLE:
        cfg, ref, imgs, labels = _inputs(depth, wseed, iseed)
        lab = labels if with_labels else None
        map32, preds32 = oracle_cam(copy.deepcopy(ref), imgs, lab, layer)
        map64, preds64 = oracle_cam(copy.deepcopy(ref).double(), imgs.double(), lab, layer)
        d0 = (map32.double() - map64).abs().max().item()
        _ORACLE[key] = dict(cfg=cfg, state=ref.state_dict(), imgs=imgs, labels=labels, map64=map64, preds32=preds32, preds64=preds64, d0=d0)
    return _ORACLE[key]


def _gpu_model(case, dev):
    import bdvcil_amd as bd
    mod = bd.build_model(copy.deepcopy(case['cfg']))
    mod.load_state_dict(case['state'])
    return mod.to(dev)


@pytest.mark.parametrize('depth,layer,wseed,iseed', MODEL_CASES)
def test_model_map_against_the_oracle(depth, layer, wseed, iseed, conv_arith, dev):
    import bdvcil_amd as bd
    case = _oracle(depth, layer, wseed, iseed)
    d0 = case['d0']
    assert 0.0 < d0 <= 1e-3, f'd0 = {d0:.3e}: the normalisation is ill-conditioned for this seed, take another'
    mod = _gpu_model(case, dev)
    out = bd.GradCAM(mod, layer)(case['imgs'].to(dev), case['labels'].to(dev))
    assert tuple(out['map'].shape) == (B_, T_, S_, S_) and tuple(out['preds'].shape) == (B_, K_CLASSES)
    perr = (out['preds'].cpu() - case['preds32']).abs().max().item()
    dist = (out['map'].cpu().double() - case['map64']).abs().max().item()
    print(f'R{depth} {layer} {conv_arith}: d0 {d0:.3e}, GPU distance to fp64 {dist:.3e} ({dist / d0:.2f} d0), logits err {perr:.2e}')
    assert perr <= 1e-3                                  # the project's bar for logits against the oracle
    assert dist <= 4 * d0                                # see the module docstring; measured ratios in profiles/gradcam.txt


def test_labels_none_takes_the_row_maximum(dev):
    import bdvcil_amd as bd
    case = _oracle(18, 'backbone.layer4', 5, 1, with_labels=False)       # seeds with a clear winner: top-2 gaps 0.055 and more
    top2 = case['preds64'].topk(2, dim=1).values
    assert ((top2[:, 0] - top2[:, 1]) > 10 * 1e-3).all(), top2        # the oracle's choice is not a coin flip at the logit bar
    mod = _gpu_model(case, dev)
    out = bd.GradCAM(mod)(case['imgs'].to(dev))
    assert torch.equal(out['labels'].cpu(), case['preds64'].argmax(1))
    assert (out['map'].cpu().double() - case['map64']).abs().max().item() <= 4 * case['d0']


def test_side_effects_and_frozen_models(dev):
    import bdvcil_amd as bd
    case = _oracle(18, 'backbone.layer4', 0, 1)
    mod = _gpu_model(case, dev)
    imgs, labels = case['imgs'].to(dev), case['labels'].to(dev)
    mod.train()
    mod.backbone.layer2.eval()                                         # a mixed pattern of flags to restore
    mod.test_cfg = dict(average_clips='prob', marker=3)
    params = list(mod.parameters())
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, 0.5) if i % 2 else None
    params[3].requires_grad_(False)
    flags = {n: m.training for n, m in mod.named_modules()}
    req = [p.requires_grad for p in params]
    bufs = {n: b.clone() for n, b in mod.named_buffers()}
    cam = bd.GradCAM(mod)
    first = cam(imgs, labels)['map']

    def unchanged():
        assert {n: m.training for n, m in mod.named_modules()} == flags
        assert mod.test_cfg == dict(average_clips='prob', marker=3)
        assert [p.requires_grad for p in params] == req
        for i, p in enumerate(params):
            assert (p.grad is None) if i % 2 == 0 else bool((p.grad == 0.5).all())
        for n, b in mod.named_buffers():
            assert torch.equal(b, bufs[n]), n                           # BatchNorm running statistics, bit for bit
        assert not mod.backbone.layer4._forward_hooks
    unchanged()

    class Boom(RuntimeError):
        pass

    def boom(_imgs):
        raise Boom()
    cam._forward = boom
    with pytest.raises(Boom):
        cam(imgs, labels)
    unchanged()
    del cam._forward
    params[3].requires_grad_(True)
    mod.eval()
    before = bd.GradCAM(mod)(imgs, labels)['map']
    mod.freeze_backbone()
    after = bd.GradCAM(mod)(imgs, labels)['map']
    assert torch.equal(before, after) and torch.equal(before, first)
    for p in mod.parameters():
        p.requires_grad_(False)
    assert torch.equal(bd.GradCAM(mod)(imgs, labels)['map'], before)    # nothing trainable at all


def test_gradcam_outputs_and_errors(dev):
    import bdvcil_amd as bd
    case = _oracle(18, 'backbone.layer4', 0, 1)
    mod = _gpu_model(case, dev)
    imgs, labels = case['imgs'].to(dev), case['labels'].to(dev)
    cam = bd.GradCAM(mod)
    boxes = [[[[8.0, 8.0, 40.0, 56.0]]] * T_, [[]] * T_]
    out = cam(imgs, labels, boxes=boxes, overlay=True, alpha=0.5)
    assert tuple(out['overlay'].shape) == (B_, T_, S_, S_, 3) and out['overlay'].dtype == torch.uint8
    att = out['actor_attention'].cpu().numpy()
    v = out['map'][0].cpu().double()
    want = (v[:, 8:56, 8:40].sum() / v.sum()).item()                    # pixel centres inside [8, 40) x [8, 56)
    assert abs(att[0] - want) <= 5 * U and np.isnan(att[1])              # no box in any frame of clip 1
    # the same input as NHWC4 frames: the same map, and the overlay reads the frames as given
    frames4 = bd.Nhwc4Frames(bd.kernels.nchw3_to_nhwc4(imgs.reshape(B_ * T_, 3, S_, S_).contiguous()), B_, T_)
    out4 = cam(frames4, labels, overlay=True)
    assert torch.equal(out4['map'], out['map']) and torch.equal(out4['overlay'], out['overlay'])
    with pytest.raises(ValueError, match='one clip per sample'):
        cam(torch.cat([imgs, imgs], 1), labels)
    with pytest.raises(ValueError, match='labels'):
        cam(imgs, torch.tensor([0, K_CLASSES]))
    with pytest.raises(TypeError, match=r'\(N, C, h, w\)'):
        bd.GradCAM(mod, 'cls_head.fc_cls')(imgs, labels)                   # a (N, K) output
    prev = bd.set_conv_arith('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16x1'):
            cam(imgs, labels)
    finally:
        bd.set_conv_arith('bf16x3')
        bd.kernels.FPROP_X3, bd.kernels.DGRAD_X3, bd.kernels.WGRAD_X3 = prev
    i3d = object.__new__(bd.Recognizer3D)                               # the constructor is not needed to be refused
    with pytest.raises(NotImplementedError, match='Recognizer3D'):
        bd.GradCAM(i3d)
    with pytest.raises(ValueError, match='colormap'):
        bd.GradCAM(mod, colormap=np.full((256, 3), 2.0))
