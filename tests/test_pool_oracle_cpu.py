"""The NumPy restatements of oracle/pool_oracle.py against torch on the CPU.  They are the references of
tests/test_pool_kernels_gpu.py, so they are held against an implementation that shares no code with them, on inputs full of ties
(values drawn from ten dyadic levels) and at the frame sizes where the window arithmetic has its edges.  Comparisons are exact
(``array_equal``) wherever both sides select values or add dyadic numbers; the two tolerances used are explained where they are
applied."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pool_oracle as P
from oracle import tsm_oracle as O

FRAMES = P.FRAMES + P.WIDE_FRAMES


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _code_to_flat_index(code, H, W):
    """uint8 tap codes (N, Ho, Wo, C) -> the flat input index hi * W + wi that F.max_pool2d(return_indices=True) reports."""
    Ho, Wo = code.shape[1:3]
    r, s = code.astype(np.int64) // 3, code.astype(np.int64) % 3
    hi = 2 * np.arange(Ho)[None, :, None, None] - 1 + r
    wi = 2 * np.arange(Wo)[None, None, :, None] - 1 + s
    assert (hi >= 0).all() and (hi < H).all() and (wi >= 0).all() and (wi < W).all()
    return hi * W + wi


def _with_special_windows(x, neg_inf):
    """Frame 0: every window tied at one value; with ``neg_inf`` a 3 x 3 corner of the last frame (the whole of window (0, 0) and
    more) is -inf."""
    x = x.copy()
    x[0] = 1.5
    if neg_inf:
        x[-1, :3, :3] = -np.inf
    return x


@pytest.mark.parametrize('H,W', FRAMES)
@pytest.mark.parametrize('neg_inf', [False, True])
def test_maxpool_values_argmax_and_backward_equal_torch(H, W, neg_inf):
    for N, C in ((1, 4), (3, 4), (2, 64)):
        x = _with_special_windows(P.dyadic((N + 1, H, W, C), 100 * H + W), neg_inf).astype(np.float64)
        out, code = P.maxpool3x3s2_first(x)
        xt = _nchw(x).requires_grad_(True)
        ref, ind = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
        assert np.array_equal(out, _nhwc(ref.detach()))
        assert np.array_equal(_code_to_flat_index(code, H, W), _nhwc(ind))
        dout = P.dyadic(out.shape, 7 * H + W).astype(np.float64)
        ref.backward(_nchw(dout))
        dx64, dx32 = P.maxpool3x3s2_bwd(dout, code, x.shape)
        assert np.array_equal(dx64, _nhwc(xt.grad))
        assert dx32.dtype == np.float32 and np.array_equal(dx32.astype(np.float64), dx64)     # dyadic terms: exact in fp32 too


def test_maxpool_first_valid_tap_on_tied_and_minus_inf_windows():
    """All-tied windows and all -inf windows take the first tap inside the frame: 4 (the centre) at the corner window, 3 on the
    top row, 1 on the left column, 0 in the interior."""
    for x in (np.full((1, 5, 5, 4), 2.0, np.float32), np.full((1, 5, 5, 4), -np.inf, np.float32)):
        out, code = P.maxpool3x3s2_first(x)
        assert np.array_equal(out, np.full((1, 3, 3, 4), x.flat[0], np.float32))
        want = np.array([[4, 3, 3], [1, 0, 0], [1, 0, 0]], np.uint8)
        assert np.array_equal(code, np.broadcast_to(want[None, :, :, None], code.shape))


def test_maxpool_fp32_ordered_backward_follows_ascending_codes():
    """Pixel (1, 1) of a 4 x 4 frame lies in all four windows, as tap 8 of (0,0), 6 of (0,1), 2 of (1,0), 0 of (1,1).  Terms chosen so
    that fp32 addition is not associative tell the orders apart: ((((0 + d11) + d10) + d01) + d00)."""
    code = np.array([[8, 6], [2, 0]], np.uint8).reshape(1, 2, 2, 1).repeat(4, axis=3)
    d = np.array([[1.0, -2.0 ** 24], [2.0 ** 24, 1.0]], np.float32).reshape(1, 2, 2, 1).repeat(4, axis=3)    # d00, d01 / d10, d11
    dx64, dx32 = P.maxpool3x3s2_bwd(d, code, (1, 4, 4, 4))
    assert (dx64[0, 1, 1] == 2.0).all()
    want = np.float32(np.float32(np.float32(np.float32(1.0) + np.float32(2.0 ** 24)) + np.float32(-2.0 ** 24)) + np.float32(1.0))
    assert want == 1.0 and (dx32[0, 1, 1] == want).all()          # 1 + 2^24 rounds to 2^24: the ordered fp32 sum is 1, not 2
    assert np.count_nonzero(dx64) == 4 and np.count_nonzero(dx32) == 4


@pytest.mark.parametrize('frame_elems', [32, 96, 7 * 7 * 64])
@pytest.mark.parametrize('frames_out', [1, 3, 513])
def test_temporal_pool_equals_torch(frame_elems, frames_out):
    if frame_elems * frames_out > 200000:
        frames_out = 33                                          # the CPU comparison needs no large case: nothing depends on the size
    x = P.dyadic((2 * frames_out, 1, frame_elems // 32, 32), frame_elems + frames_out).astype(np.float64)
    out, sel = P.maxpool_t2(x)
    xt = torch.from_numpy(x).permute(3, 0, 1, 2)[None].contiguous().requires_grad_(True)      # (1, C, T, H, W)
    ref = F.max_pool3d(xt, (2, 1, 1), (2, 1, 1))
    assert np.array_equal(out, ref.detach()[0].permute(1, 2, 3, 0).numpy())
    dout = P.dyadic(out.shape, 3).astype(np.float64)
    ref.backward(torch.from_numpy(dout).permute(3, 0, 1, 2)[None].contiguous())
    dx = P.maxpool_t2_bwd(dout, sel)
    assert np.array_equal(dx, xt.grad[0].permute(1, 2, 3, 0).numpy())
    bits = P.unpack_bits(sel, out.shape)
    assert np.array_equal(bits, x[1::2] > x[0::2]) and bits.any() and not bits.all()
    assert (dx[0::2][bits] == 0).all() and (dx[1::2][~bits] == 0).all()       # the losing frame gets exactly 0
    assert (x[0::2] == x[1::2]).mean() > 0.05                                  # ties are frequent, and they go to frame 2t
    assert not bits[x[0::2] == x[1::2]].any()


@pytest.mark.parametrize('HW', [1, 4, 49, 50])
@pytest.mark.parametrize('C', [4, 64, 2048])
def test_avgpool_restatements(HW, C):
    for N in (1, 5):
        x = np.random.default_rng(HW * C + N).standard_normal((N, HW, 1, C)).astype(np.float32)
        m64, m32 = P.avgpool(x)
        ref = F.adaptive_avg_pool2d(_nchw(x).double(), 1)[:, :, 0, 0].numpy()
        # fp64 against fp64: summation order only
        assert np.abs(m64 - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        # HW additions and one multiply, each of relative error 2^-24, against the exact mean
        bound = (HW + 1) * 2.0 ** -24 * np.abs(x.astype(np.float64)).mean(axis=(1, 2))
        assert m32.dtype == np.float32 and (np.abs(m32.astype(np.float64) - m64) <= bound).all()
        d = np.random.default_rng(C).standard_normal((N, C)).astype(np.float32)
        dx = P.avgpool_bwd(d, HW)
        assert dx.shape == (N, HW, C) and np.array_equal(dx, np.broadcast_to((d * (np.float32(1) / np.float32(HW)))[:, None], dx.shape))
        xt = torch.from_numpy(x.reshape(N, HW, C)).double().requires_grad_(True)
        xt.mean(dim=1).backward(torch.from_numpy(d).double())
        assert np.abs(dx - xt.grad.numpy()).max() <= 2.0 ** -23 * max(np.abs(d).max() / HW, 1e-30)    # rounding of 1/HW and of the product


@pytest.mark.parametrize('H,W', FRAMES)
def test_stem_tail_and_backward_equal_torch_fp64(H, W):
    """relu(batch_norm(y)) -> max_pool2d -> autograd in fp64 against stem_tail + stem_backward.  torch normalises as
    (y - mean) * invstd * gamma + beta, the restatement as y * scale + shift: the two differ by fp64 rounding, hence values at 1e-12
    and gradients at 1e-10 of scale; arg-max positions and the mask are compared exactly (tied inputs stay tied in both forms)."""
    for N, C in ((1, 32), (3, 64)):
        y = P.dyadic((N, H, W, C), 11 * H + W)
        gamma, beta = P.dyadic_affine(C, H + 13 * W)
        y64 = y.astype(np.float64)
        mean, var = y64.mean(axis=(0, 1, 2)), y64.var(axis=(0, 1, 2))
        invstd = 1.0 / np.sqrt(var + 1e-5)
        scale = gamma.astype(np.float64) * invstd
        shift = beta.astype(np.float64) - mean * scale
        pooled, code, mask = P.stem_tail(y, scale, shift)
        yt = _nchw(y64).requires_grad_(True)
        gt = torch.from_numpy(gamma).double().requires_grad_(True)
        bt = torch.from_numpy(beta).double().requires_grad_(True)
        a = F.relu(F.batch_norm(yt, None, None, gt, bt, training=True, eps=1e-5))
        ref, ind = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        assert np.abs(pooled - _nhwc(ref.detach())).max() <= 1e-12 * max(1.0, np.abs(pooled).max())
        assert np.array_equal(_code_to_flat_index(code, H, W), _nhwc(ind))
        assert np.array_equal(P.unpack_bits(mask, y.shape), _nhwc(a.detach()) > 0)
        dpool = P.dyadic(pooled.shape, H * W)
        ref.backward(_nchw(dpool.astype(np.float64)))
        dy, dgamma, dbeta = P.stem_backward(dpool, code, mask, y, gamma, mean, invstd)
        for got, want in ((dy, _nhwc(yt.grad)), (dgamma, gt.grad.numpy()), (dbeta, bt.grad.numpy())):
            assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
        assert (scale[0] == 0) and (code[..., 0] == P.maxpool3x3s2_first(np.zeros_like(y))[1][..., 0]).all()   # scale 0: first valid tap


def test_affine_then_max_differs_from_max_then_affine():
    """The inputs carry what tells the two apart: on negative-scale channels pooling y first picks the wrong tap."""
    y = P.dyadic((3, 9, 8, 32), 5)
    scale, shift = P.dyadic_affine(32, 6)
    pooled, code, _ = P.stem_tail(y, scale, shift)
    m, mcode = P.maxpool3x3s2_first(y)
    swapped = np.maximum(m.astype(np.float64) * scale + shift, 0)
    neg = scale < 0
    assert neg.any() and (scale == 0).any()
    assert (swapped[..., neg] != pooled[..., neg]).mean() > 0.2 and (mcode[..., neg] != code[..., neg]).mean() > 0.2


@pytest.mark.parametrize('shape,seed', P.STEM_RANDN_CASES)
def test_family_b_stem_inputs_leave_the_rounding_band_nearly_empty(shape, seed):
    """tests/test_pool_kernels_gpu.py compares the ReLU mask of randn inputs only where |y * scale + shift| exceeds the rounding
    band e, and asserts that at most 0.1 % of the tensor lies inside it.  That is a property of the inputs: established here for the
    very tensors (same generator, same seeds) the GPU test uses."""
    y, scale, shift = P.randn_stem_case(shape, seed)
    aff, e = P.stem_affine(y, scale, shift), P.stem_band(y, scale, shift)
    inside = np.abs(aff) <= e
    assert inside.mean() <= 1e-3
    assert (scale == 0).any() and (scale < 0).any()


def _splitmix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


@pytest.mark.parametrize('seed', [0, 1234, 2 ** 63 + 5])
def test_dropout_mask_against_python_integers_and_for_independence(seed):
    """The uint64 NumPy arithmetic (wrap-around included: seed 2^63 + 5 overflows the product) against Python's integers, the keep
    rate, and the correlation of neighbouring elements (5 sigma of a fair Bernoulli sequence)."""
    n = 1 << 16
    for p in (0.0, 0.5, 0.8, 0.999):
        keep, scale = P.dropout_mask(n, p, seed)
        for i in (0, 1, 255, 256, n - 1):
            h = _splitmix64((seed * 0xD1342543DE82EF95 + i) & ((1 << 64) - 1))
            assert bool(keep[i]) == (np.float32((h >> 40) * 2.0 ** -24) >= np.float32(p))
        assert scale == np.float32(1) / (np.float32(1) - np.float32(p))
        q = 1.0 - float(np.float32(p))
        assert abs(keep.mean() - q) <= 5 * np.sqrt(q * (1 - q) / n) + 2.0 ** -24
        if 0 < q < 1:
            for lag in (1, 2, 64, 256):
                a, b = keep[:-lag].astype(np.float64) - q, keep[lag:].astype(np.float64) - q
                assert abs((a * b).mean()) <= 5 * q * (1 - q) / np.sqrt(n - lag)
    assert P.dropout_mask(n, 0.0, seed)[0].all()
    assert not np.array_equal(P.dropout_mask(n, 0.5, seed)[0], P.dropout_mask(n, 0.5, seed + 1)[0])


@pytest.mark.parametrize('alpha', [0.5, 0.3])
def test_bgmix_with_a_float_background_restates_the_uint8_one(alpha):
    """On a background of whole grey levels the fp32-background restatement is the uint8 one bit for bit (alpha = 0.3: the blend
    weights are fp32(0.3) and 1 - fp32(0.3) in both), in both layouts."""
    g = torch.Generator().manual_seed(5)
    B, T, H, W = 3, 2, 5, 7
    fr = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    bg = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    mix = torch.tensor([True, False, True])
    o4, oc = O.bgmix_normalize_f32bg(fr, bg.float(), mix, alpha)
    assert torch.equal(oc, O.bgmix_normalize(fr, bg, mix, alpha))
    assert torch.equal(o4[..., :3].reshape(B, T, H, W, 3).permute(0, 1, 4, 2, 3), oc)
    assert torch.equal(o4[..., 3], torch.zeros(B * T, H, W)) and not torch.signbit(o4[..., 3]).any()
