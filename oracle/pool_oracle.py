"""Plain NumPy restatements of the small HBM-bound operations around the conv stack: MaxPool2d(3, 2, 1) with arg-max codes and
its backward, the fused stem tail (BatchNorm apply + ReLU + max-pool + 1-bit ReLU mask) and the BatchNorm backward behind it, the
temporal max-pool of I3D, the global average pool, and the counter-based dropout mask.

Each function is written from the operation's definition (tests/test_pool_oracle_cpu.py holds them against torch on the CPU) and
is the reference of tests/test_pool_kernels_gpu.py.  Tensors are NHWC NumPy arrays; N and C are vectorised, the nine taps and the
pixels of an average are Python loops.

Bit layouts shared with the kernels:
  * ``code``: uint8 per pooled element, r * 3 + s of the window tap that was taken (window row r, column s, 0..2);
  * bit masks (ReLU mask, temporal-pool ``sel``): 1 bit per element in flat NHWC order, bit k of int32 word w = element 32 w + k.
"""
import numpy as np


def out_size(n: int) -> int:
    """Output length of a (3, 2, 1) pooling window over n inputs."""
    return (n + 2 - 3) // 2 + 1


def pack_bits(bits) -> np.ndarray:
    """bool array (numel % 32 == 0) -> int32 words, element 32 w + k in bit k of word w."""
    flat = np.ascontiguousarray(bits, dtype=bool).reshape(-1)
    assert flat.size % 32 == 0, flat.size
    return np.packbits(flat, bitorder='little').view('<i4').astype(np.int32)


def unpack_bits(words, shape) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.int32).astype('<i4')
    return np.unpackbits(w.view(np.uint8), bitorder='little').astype(bool).reshape(shape)


def _tap_ranges(n_in: int, n_out: int, k: int):
    """Outputs o in [o0, o1) whose tap k (input 2 o - 1 + k) lies inside the frame, and the input slice they read."""
    o0 = 1 if k == 0 else 0
    o1 = min(n_out, (n_in - k) // 2 + 1)
    return o0, o1, slice(2 * o0 - 1 + k, 2 * o1 - 2 + k, 2)


def maxpool3x3s2_first(x):
    """MaxPool2d(3, 2, 1) of x (N, H, W, C) -> (out, code).  Taps are scanned in (r, s) order, a tap outside the frame is skipped,
    and a tap is taken when nothing has been taken yet or its value is strictly greater: the first maximum wins, and a window of
    -inf only keeps its first valid tap."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = out_size(H), out_size(W)
    out = np.zeros((N, Ho, Wo, C), x.dtype)
    code = np.full((N, Ho, Wo, C), 255, np.uint8)
    for r in range(3):
        h0, h1, hs = _tap_ranges(H, Ho, r)
        if h1 <= h0:
            continue
        for s in range(3):
            w0, w1, ws = _tap_ranges(W, Wo, s)
            if w1 <= w0:
                continue
            tap = x[:, hs, ws]
            o, c = out[:, h0:h1, w0:w1], code[:, h0:h1, w0:w1]
            take = (c == 255) | (tap > o)
            o[take] = tap[take]
            c[take] = r * 3 + s
    assert (code != 255).all()          # every window of a frame with H, W >= 1 holds its centre tap
    return out, code


def maxpool3x3s2_bwd(dout, code, in_shape):
    """Scatter-add of dout (N, Ho, Wo, C) to the tap each code names -> (dx in fp64, dx in fp32).  The fp32 result adds an input
    pixel's contributions (at most four windows cover a pixel) in ascending code order starting from +0, the order the gather
    of the kernels documents (csrc/common.h, pool_bwd_gather2x2)."""
    dout, code = np.asarray(dout), np.asarray(code)
    N, H, W, C = in_shape
    Ho, Wo = out_size(H), out_size(W)
    assert dout.shape == (N, Ho, Wo, C) and code.shape == dout.shape
    d64, d32 = dout.astype(np.float64), dout.astype(np.float32)
    dx64 = np.zeros((N, H, W, C), np.float64)
    dx32 = np.zeros((N, H, W, C), np.float32)
    for r in range(3):
        h0, h1, hs = _tap_ranges(H, Ho, r)
        if h1 <= h0:
            continue
        for s in range(3):
            w0, w1, ws = _tap_ranges(W, Wo, s)
            if w1 <= w0:
                continue
            sel = code[:, h0:h1, w0:w1] == r * 3 + s
            # one tap of distinct windows never names the same pixel twice (stride 2): a sliced += is a scatter without collisions
            dx64[:, hs, ws] += np.where(sel, d64[:, h0:h1, w0:w1], 0.0)
            t32 = dx32[:, hs, ws]
            dx32[:, hs, ws] = np.where(sel, t32 + d32[:, h0:h1, w0:w1], t32)
    return dx64, dx32


def stem_tail(y, scale, shift):
    """a = max(y * scale + shift, 0) in fp64, then MaxPool2d(3, 2, 1) of a -> (pooled fp64, code, mask_bits); mask_bits = a > 0,
    packed (``pack_bits``)."""
    a = stem_activation(y, scale, shift)
    pooled, code = maxpool3x3s2_first(a)
    return pooled, code, pack_bits(a > 0)


def stem_affine(y, scale, shift):
    """y * scale + shift per channel, in fp64."""
    return np.asarray(y, dtype=np.float64) * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64)


def stem_activation(y, scale, shift):
    return np.maximum(stem_affine(y, scale, shift), 0.0)


def maxpool_t2(x):
    """MaxPool3d((2,1,1), (2,1,1)) over frames: x (2n, ...) -> (out (n, ...), sel_bits).  The larger of frames 2t and 2t+1, ties to
    frame 2t; sel bit set when frame 2t+1 won."""
    x = np.asarray(x)
    a, b = x[0::2], x[1::2]
    sel = b > a
    return np.where(sel, b, a), pack_bits(sel)


def maxpool_t2_bwd(dout, sel_bits):
    dout = np.asarray(dout)
    sel = unpack_bits(sel_bits, dout.shape)
    dx = np.zeros((2 * dout.shape[0],) + dout.shape[1:], dout.dtype)
    dx[0::2] = np.where(sel, 0, dout)
    dx[1::2] = np.where(sel, dout, 0)
    return dx


def avgpool(x):
    """x (N, H, W, C) or (N, HW, C) -> (mean in fp64, fp32 restatement): the fp32 one adds the pixels sequentially in pixel order
    in fp32, then multiplies once by float32(1) / float32(HW)."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    HW = x.shape[1]
    s = np.zeros((x.shape[0], x.shape[2]), np.float32)
    x32 = x.astype(np.float32)
    for p in range(HW):
        s = s + x32[:, p]
    inv = np.float32(1) / np.float32(HW)
    return x.astype(np.float64).mean(axis=1), s * inv


def avgpool_bwd(d, HW):
    """d (N, C) -> (N, HW, C): d * float32(1 / HW) for every pixel."""
    d = np.asarray(d, dtype=np.float32)
    inv = np.float32(1) / np.float32(HW)
    return np.broadcast_to((d * inv)[:, None, :], (d.shape[0], HW, d.shape[1])).copy()


_M64 = (1 << 64) - 1


def dropout_mask(numel: int, p: float, seed: int):
    """-> (keep (numel,) bool, scale float32).  h = splitmix64(seed * 0xD1342543DE82EF95 + i) in uint64 with wrap-around,
    u = (h >> 40) * 2**-24, keep when float32(u) >= float32(p); scale = float32(1) / (float32(1) - float32(p))."""
    base = np.uint64(((int(seed) & _M64) * 0xD1342543DE82EF95) & _M64)
    with np.errstate(over='ignore'):
        z = np.arange(numel, dtype=np.uint64) + base            # wraps modulo 2**64
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = z ^ (z >> np.uint64(31))
    u = (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)        # 24 bits: exact in fp32
    keep = u >= np.float32(p)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    return keep, scale


def stem_backward(dpool, code, mask_bits, y, gamma, mean, invstd):
    """BatchNorm(+ReLU) backward behind MaxPool2d(3, 2, 1), all in fp64 -> (dy, dgamma, dbeta):
    g = relu-mask * maxpool3x3s2_bwd(dpool, code); dbeta = sum g; dgamma = sum g * xhat; dy = gamma * invstd * (g - dbeta / M -
    xhat * dgamma / M) with xhat = (y - mean) * invstd and M = N * H * W."""
    y64 = np.asarray(y, dtype=np.float64)
    N, H, W, C = y64.shape
    M = N * H * W
    g = maxpool3x3s2_bwd(dpool, code, y64.shape)[0] * unpack_bits(mask_bits, y64.shape)
    mean, invstd, gamma = (np.asarray(t, dtype=np.float64) for t in (mean, invstd, gamma))
    xhat = (y64 - mean) * invstd
    dbeta = g.sum(axis=(0, 1, 2))
    dgamma = (g * xhat).sum(axis=(0, 1, 2))
    dy = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    return dy, dgamma, dbeta


def window_taps(x, fill):
    """The nine taps of every MaxPool2d(3, 2, 1) window of x (N, H, W, C) -> (9, N, Ho, Wo, C), tap r * 3 + s first; a tap outside
    the frame holds ``fill``."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = out_size(H), out_size(W)
    taps = np.full((9, N, Ho, Wo, C), fill, x.dtype)
    for r in range(3):
        h0, h1, hs = _tap_ranges(H, Ho, r)
        for s in range(3):
            w0, w1, ws = _tap_ranges(W, Wo, s)
            if h1 > h0 and w1 > w0:
                taps[r * 3 + s, :, h0:h1, w0:w1] = x[:, hs, ws]
    return taps


# ---- seeded inputs of the tests (shared by the CPU and the GPU test files, so that what the CPU file establishes about an input
# ---- holds for the tensor the kernels see) ------------------------------------------------------------------------------------

_LEVELS = np.array([-4, -3, -1.5, -0.625, -0.125, 0, 0.125, 0.75, 2, 4], np.float32)      # multiples of 1/8 in [-4, 4]


def dyadic(shape, seed) -> np.ndarray:
    """fp32 values drawn from ten multiples of 1/8 in [-4, 4]: ties in almost every 3 x 3 window, and sums of a few of them, or of
    their products with the scales below, are exact in fp32 with or without fused multiply-add."""
    return _LEVELS[np.random.default_rng(seed).integers(0, len(_LEVELS), size=shape)]


def dyadic_affine(C, seed):
    """(scale, shift) fp32: scale a multiple of 1/4 in [-2, 2] with channel 0 exactly 0 and channel 1 negative (where "affine, ReLU,
    then max" and "max, then affine" differ), shift a multiple of 1/8 in [-2, 2]."""
    rng = np.random.default_rng(seed)
    scale = (rng.integers(-8, 9, size=C) / 4).astype(np.float32)
    shift = (rng.integers(-16, 17, size=C) / 8).astype(np.float32)
    scale[0], scale[1 % C] = 0.0, -1.25
    scale[2 % C] = -0.5 if C > 2 else scale[2 % C]
    return scale, shift


def randn_stem_case(shape, seed):
    """Family (b) input of the stem tail: (y, scale, shift) fp32 from a normal distribution; scale keeps its zero and negative
    channels."""
    rng = np.random.default_rng(seed)
    C = shape[-1]
    y = rng.standard_normal(shape).astype(np.float32)
    scale = rng.standard_normal(C).astype(np.float32)
    shift = rng.standard_normal(C).astype(np.float32)
    scale[0], scale[1] = 0.0, -abs(scale[1]) - 0.25
    return y, scale, shift


def stem_band(y, scale, shift):
    """e = 2**-23 * (|y * scale| + |shift|): the two roundings of an fp32 multiply and add (one with a fused multiply-add), each of
    relative error 2**-24, against the fp64 value."""
    y64 = np.asarray(y, dtype=np.float64)
    return 2.0 ** -23 * (np.abs(y64 * np.asarray(scale, dtype=np.float64)) + np.abs(np.asarray(shift, dtype=np.float64)))


# (N, H, W) frames of the 2-D pooling tests: every parity of H and W, frames smaller than a window, and two rows wide enough
# (Wo * C / 4 > 256 at C = 64) for a second block along x with a ragged tail
FRAMES = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (5, 4), (7, 7), (8, 9), (9, 8), (16, 15)]
WIDE_FRAMES = [(6, 40), (5, 37)]          # C = 64 only
# (shape, seed) of the family (b) stem-tail inputs: C = 64, 128, the forward-only 96, and a row two blocks wide
STEM_RANDN_CASES = [((3, 16, 15, 64), 21), ((3, 9, 8, 128), 22), ((1, 7, 7, 96), 23), ((3, 5, 37, 64), 24)]


def bn_stem_case(shape, seed):
    """Input of the stem backward: dyadic y (ties), gamma with a zero and negative channels, beta, the fp64 batch statistics of y
    rounded to fp32 (what the backward kernel is handed), and the forward's fp32 (scale, shift) derived from them in fp64."""
    y = dyadic(shape, seed)
    gamma, beta = dyadic_affine(shape[-1], seed + 1)
    y64 = y.astype(np.float64)
    mean = y64.mean(axis=(0, 1, 2)).astype(np.float32)
    invstd = (1.0 / np.sqrt(y64.var(axis=(0, 1, 2)) + 1e-5)).astype(np.float32)
    scale = (gamma.astype(np.float64) * invstd).astype(np.float32)
    shift = (beta.astype(np.float64) - mean.astype(np.float64) * scale).astype(np.float32)
    return y, gamma, beta, mean, invstd, scale, shift
