"""Edge sweep of the small HBM-bound kernels -- csrc/pool_frontend.hip, relu_bwd / add / bn_bwd_pool in csrc/bn.hip, dropout in
csrc/head_loss.hip -- against the NumPy restatements of oracle/pool_oracle.py (held against torch in tests/test_pool_oracle_cpu.py),
never against a sibling kernel.

Pooling selects values, the backward gather adds at most four terms in a documented order, and on inputs from a coarse dyadic grid
(family (a): multiples of 1/8, scales multiples of 1/4) every product and sum is exact in fp32 with or without fused multiply-add.
So the comparisons are ``torch.equal`` / ``array_equal``.  The tolerances that remain are derived where they are applied:
  * the two-rounding band e of an fp32 multiply-add on randn data (stem tail, family (b));
  * the BatchNorm backward bars of test_ops_gpu.py::test_bn_train_fwd_bwd (reductions over the batch in fp32 / fp64).

Outputs are allocated inside the wrappers with ``torch.empty`` and cannot be prefilled.  As a best effort ``_poison`` runs after the
inputs are on the device and right before a call: it fills and frees blocks of the outputs' sizes with 0xFF (NaN as fp32 / bf16,
code 255, mask -1), which the caching allocator will usually hand to the wrapper next, so that an element the kernel does not write
is unlikely to hold the correct result of an earlier identical call.  Nothing rests on it: the whole output is compared with the
reference either way."""
import numpy as np
import pytest
import torch

from oracle import pool_oracle as P
from oracle import tsm_oracle as O

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _k():
    from bdvcil_amd import kernels as K
    return K


def _t(a, dev=None, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t if dev is None else t.to(dev)


def _poison(dev, *tensors_like):
    """Fill and free one block per (shape, dtype) about to be allocated (best effort, see the module docstring).  Call it after every
    input of the kernel call is on the device, so that no upload takes the freed block."""
    blocks = [torch.full((int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev)
              for shape, dtype in tensors_like]
    torch.cuda.synchronize()
    del blocks


def _eq(got, want, what=''):
    """Exact: same shape, same dtype, same values (-inf equals -inf; +0 equals -0, as for torch.equal)."""
    got = got.cpu() if isinstance(got, torch.Tensor) else _t(got)
    want = want if isinstance(want, torch.Tensor) else _t(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | (got != got)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {got.numel()} elements differ, first at {i}: got {got[tuple(i)].item()}, '
                             f'want {want[tuple(i)].item()}')


def _special(x, neg_inf):
    """The left half of frame 0 holds one value: every window inside it is tied.  neg_inf: the last three rows and columns of the
    last frame -- its last window entirely, and all of a 2 x 2 or 3 x 3 frame -- are -inf."""
    x = x.copy()
    x[0, :, :(x.shape[2] + 1) // 2] = 1.5
    if neg_inf:
        x[-1, -3:, -3:] = -np.inf
    return x


def _pool_cases(H, W, channels):
    wide = (H, W) in P.WIDE_FRAMES
    for N in (1, 3):
        for C in ((64,) if wide else channels):
            yield N, C


ALL_FRAMES = P.FRAMES + P.WIDE_FRAMES


# ---- MaxPool2d(3, 2, 1) --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W', ALL_FRAMES)
def test_maxpool_fwd_values_and_codes(H, W, dev):
    K = _k()
    for N, C in _pool_cases(H, W, (4, 64)):
        inputs = {'dyadic': _special(P.dyadic((N, H, W, C), 31 * H + W), False),
                  'dyadic, -inf windows': _special(P.dyadic((N, H, W, C), 31 * H + W + 1), True),
                  'randn': np.random.default_rng(H * W + C).standard_normal((N, H, W, C)).astype(np.float32)}
        for name, x in inputs.items():
            what = f'{name} {x.shape}'
            ref, code = P.maxpool3x3s2_first(x)
            xd = _t(x, dev)
            _poison(dev, (ref.shape, torch.float32), (ref.shape, torch.uint8))
            out, idx = K.maxpool_fwd(xd)
            _eq(out, ref, what + ' values')
            _eq(idx, code, what + ' codes')
            _poison(dev, (ref.shape, BF16), (ref.shape, torch.uint8))
            outb, idxb = K.maxpool_fwd(xd, BF16)
            _eq(outb, _t(ref).to(BF16), what + ' bf16 values')          # one rounding of the selected value
            _eq(idxb, code, what + ' bf16 codes')


@pytest.mark.parametrize('H,W', ALL_FRAMES)
def test_maxpool_bwd_from_the_restatements_codes(H, W, dev):
    """The codes come from the restatement (uploaded), not from the kernel under test.  Dyadic gradients: the fp64 scatter, exactly.
    randn gradients: the fp32 sum in ascending code order starting from +0 (csrc/common.h, pool_bwd_gather2x2), exactly.  The whole
    of dx is compared with the reference, the last row and column of an odd frame included."""
    K = _k()
    for N, C in _pool_cases(H, W, (4, 64)):
        shape = (N, H, W, C)
        _, code = P.maxpool3x3s2_first(_special(P.dyadic(shape, 17 * H + W), False))
        coded = _t(code, dev)
        d_a = P.dyadic(code.shape, H + 19 * W)
        d_b = np.random.default_rng(H + W + C).standard_normal(code.shape).astype(np.float32)
        d_bf = _t(d_b).to(BF16)
        d_ad, d_bd, d_bfd, d_bfwd = _t(d_a, dev), _t(d_b, dev), d_bf.to(dev), d_bf.float().to(dev)
        dx64, _ = P.maxpool3x3s2_bwd(d_a, code, shape)
        _poison(dev, (shape, torch.float32))
        _eq(K.maxpool_bwd(d_ad, coded, shape), dx64.astype(np.float32), f'dyadic {shape}')
        assert np.array_equal(dx64.astype(np.float32).astype(np.float64), dx64)
        _poison(dev, (shape, torch.float32))
        _eq(K.maxpool_bwd(d_bd, coded, shape), P.maxpool3x3s2_bwd(d_b, code, shape)[1], f'randn {shape}')
        # bf16 storage of dout: the result of its fp32 widening
        _poison(dev, (shape, torch.float32))
        got = K.maxpool_bwd(d_bfd, coded, shape)
        _eq(got, P.maxpool3x3s2_bwd(d_bf.float().numpy(), code, shape)[1], f'bf16 dout {shape}')
        _poison(dev, (shape, torch.float32))
        _eq(got, K.maxpool_bwd(d_bfwd, coded, shape).cpu(), f'bf16 dout against its widening {shape}')


def test_maxpool_row_loop(dev):
    """N * Ho = 65600 rows exceed the grid.y cap of 65535: the ``row += gridDim.y`` loop of both kernels runs a second time."""
    K = _k()
    shape = (32800, 4, 4, 4)
    assert shape[0] * P.out_size(shape[1]) >= 65536 + 64
    x = P.dyadic(shape, 71)
    ref, code = P.maxpool3x3s2_first(x)
    xd = _t(x, dev)
    _poison(dev, (ref.shape, torch.float32), (ref.shape, torch.uint8))
    out, idx = K.maxpool_fwd(xd)
    _eq(out, ref, 'values')
    _eq(idx, code, 'codes')
    d = P.dyadic(code.shape, 72)
    dd, coded = _t(d, dev), _t(code, dev)
    _poison(dev, (shape, torch.float32))
    _eq(K.maxpool_bwd(dd, coded, shape), P.maxpool3x3s2_bwd(d, code, shape)[0].astype(np.float32), 'dx')


# ---- stem tail: BatchNorm apply + ReLU + MaxPool2d(3, 2, 1) + ReLU mask ---------------------------------------------------

def _stem_fwd_exact(K, dev, y, scale, shift, what):
    pooled, code, mask = P.stem_tail(y, scale, shift)
    p32 = pooled.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), pooled)           # family (a): the fp64 result is an fp32 number
    yd, sd, bd = _t(y, dev), _t(scale, dev), _t(shift, dev)
    _poison(dev, (p32.shape, torch.float32), (p32.shape, torch.uint8), ((y.size // 32,), torch.int32))
    out, idx, m = K.bn_relu_maxpool_fwd(yd, sd, bd)
    _eq(out, p32, what + ' pooled')
    _eq(idx, code, what + ' codes')
    _eq(m, mask, what + ' mask')
    _poison(dev, (p32.shape, BF16), (p32.shape, torch.uint8), ((y.size // 32,), torch.int32))
    outb, idxb, mb = K.bn_relu_maxpool_fwd(yd, sd, bd, BF16)
    _eq(outb, out.cpu().to(BF16), what + ' bf16 pooled')
    _eq(idxb, code, what + ' bf16 codes')
    _eq(mb, mask, what + ' bf16 mask')
    return code


@pytest.mark.parametrize('H,W', ALL_FRAMES)
def test_stem_tail_dyadic(H, W, dev):
    """Family (a), exact.  Channel 0 has scale 0 (every window tied: the code must be the first tap inside the frame), channels 1
    and 2 a negative scale (the arg-max of relu(affine(y)) is not the arg-max of y)."""
    K = _k()
    for N, C in list(_pool_cases(H, W, (32, 64, 128))) + ([] if (H, W) in P.WIDE_FRAMES else [(1, 96)]):
        y = _special(P.dyadic((N, H, W, C), 41 * H + W + C), False)
        scale, shift = P.dyadic_affine(C, 43 * H + W + C)
        assert (scale == 0).any() and (scale < 0).any()
        code = _stem_fwd_exact(K, dev, y, scale, shift, f'{y.shape}')
        assert np.array_equal(code[..., 0], P.maxpool3x3s2_first(np.zeros_like(y))[1][..., 0])


def test_stem_tail_row_loop(dev):
    """N * Ho = 65600 > 65535: the fused kernel's row loop runs a second time (67 MB of input)."""
    shape = (32800, 4, 4, 32)
    assert shape[0] * P.out_size(shape[1]) >= 65536 + 64
    scale, shift = P.dyadic_affine(32, 82)
    _stem_fwd_exact(_k(), dev, P.dyadic(shape, 81), scale, shift, f'{shape}')


@pytest.mark.parametrize('shape,seed', P.STEM_RANDN_CASES)
def test_stem_tail_randn(shape, seed, dev):
    """Family (b): products and sums round.  e = 2^-23 (|y scale| + |shift|) bounds the fp32 value of y * scale + shift against fp64
    (a multiply and an add of relative error 2^-24 each, or one fused rounding); max(., 0) and the selection add no error.
      1. |out - ref64| <= e, e taken at the reference's arg-max;
      2. the kernel's code names a tap inside the frame whose activation is within e of the output, and no tap of the window exceeds
         the output by more than its own e;
      3. the mask bit equals a64 > 0 wherever |y * scale + shift| > e; at most 0.1 % of the tensor lies inside the band
         (tests/test_pool_oracle_cpu.py establishes that for these very inputs)."""
    K = _k()
    y, scale, shift = P.randn_stem_case(shape, seed)
    aff, e = P.stem_affine(y, scale, shift), P.stem_band(y, scale, shift)
    a64 = np.maximum(aff, 0.0)
    pooled, code, _ = P.stem_tail(y, scale, shift)
    yd, sd, bd = _t(y, dev), _t(scale, dev), _t(shift, dev)
    _poison(dev, (pooled.shape, torch.float32), (pooled.shape, torch.uint8), ((y.size // 32,), torch.int32))
    out_t, idx_t, mask_t = K.bn_relu_maxpool_fwd(yd, sd, bd)
    out, idx, mask = out_t.cpu().numpy().astype(np.float64), idx_t.cpu().numpy(), mask_t.cpu().numpy()
    taps_a, taps_e = P.window_taps(a64, -np.inf), P.window_taps(e, 0.0)
    pick = lambda taps, c: np.take_along_axis(taps, c[None].astype(np.int64), axis=0)[0]       # noqa: E731
    assert idx.max() <= 8
    a_k, e_k, e_ref = pick(taps_a, idx), pick(taps_e, idx), pick(taps_e, code)
    assert np.isfinite(a_k).all(), 'a code names a tap outside the frame'
    assert (np.abs(out - pooled) <= e_ref).all(), np.abs(out - pooled).max()
    assert (np.abs(a_k - out) <= e_k).all()
    assert (taps_a - out[None] <= taps_e).all()
    bits = P.unpack_bits(mask, y.shape)
    clear = np.abs(aff) > e
    assert (~clear).mean() <= 1e-3
    assert np.array_equal(bits[clear], (a64 > 0)[clear])
    # scale 0: the activation is relu(shift) everywhere, nothing rounds, and the code is the first tap inside the frame
    assert np.array_equal(idx[..., 0], P.maxpool3x3s2_first(np.zeros_like(y))[1][..., 0])
    assert np.array_equal(out[..., 0], pooled[..., 0])
    _poison(dev, (pooled.shape, BF16), (pooled.shape, torch.uint8), ((y.size // 32,), torch.int32))
    outb, idxb, maskb = K.bn_relu_maxpool_fwd(yd, sd, bd, BF16)
    _eq(outb, out_t.cpu().to(BF16), 'bf16 pooled')
    _eq(idxb, idx_t.cpu(), 'bf16 codes')
    _eq(maskb, mask_t.cpu(), 'bf16 mask')


def test_stem_backward_refuses_96_channels(dev):
    """The forward takes any C % 32 == 0; the backward's block reduction needs 256 % (C / 4) == 0 and must say so."""
    K = _k()
    y, gamma, beta, mean, invstd, scale, shift = P.bn_stem_case((1, 7, 7, 96), 5)
    out, idx, mask = K.bn_relu_maxpool_fwd(_t(y, dev), _t(scale, dev), _t(shift, dev))
    with pytest.raises((ValueError, RuntimeError)):
        K.bn_backward_maxpool(torch.zeros_like(out), idx, mask, _t(y, dev), _t(gamma, dev), _t(mean, dev), _t(invstd, dev))
    torch.cuda.synchronize()


def _bn_close(got, want, atol, what):
    """The bars of test_ops_gpu.py::test_bn_train_fwd_bwd: max error within 2e-5 of the reference's largest magnitude, plus 1e-6
    (dy) or 1e-4 (dgamma / dbeta, sums over the batch)."""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    assert err <= 2e-5 * scale + atol, f'{what}: max err {err} vs scale {scale}'


def _stem_bwd(K, dev, shape, seed):
    y, gamma, beta, mean, invstd, scale, shift = P.bn_stem_case(shape, seed)
    pooled, code, mask = P.stem_tail(y, scale, shift)
    dpool = P.dyadic(pooled.shape, seed + 2)              # multiples of 1/8 up to 4: bf16 holds them exactly
    dy, dgamma, dbeta = P.stem_backward(dpool, code, mask, y, gamma, mean, invstd)
    args = [_t(a, dev) for a in (code, mask, y, gamma, mean, invstd)]
    for dt in (torch.float32, BF16):
        for splits in (0, 1):
            what = f'{shape} dpool {dt} splits {splits}'
            dpd = _t(dpool, dev, dt)
            _poison(dev, (shape, torch.float32))
            g_dy, g_dg, g_db = K.bn_backward_maxpool(dpd, *args, splits=splits)
            _bn_close(g_dy, dy, 1e-6, what + ' dy')
            _bn_close(g_dg, dgamma, 1e-4, what + ' dgamma')
            _bn_close(g_db, dbeta, 1e-4, what + ' dbeta')


@pytest.mark.parametrize('H,W', ALL_FRAMES)
def test_stem_backward_against_fp64_chain(H, W, dev):
    """Codes and mask from the restatement, mean / invstd from fp64 statistics rounded to fp32; dy, dgamma, dbeta against the fp64
    chain g = mask * pool_bwd(dpool), dbeta = sum g, dgamma = sum g xhat, dy = gamma invstd (g - dbeta / M - xhat dgamma / M)."""
    K = _k()
    for N, C in _pool_cases(H, W, (32, 64, 128)):
        _stem_bwd(K, dev, (N, H, W, C), 53 * H + W + C)


def test_stem_backward_row_loop(dev):
    """N * Ho = 4200 > 4096 rows of grid.y: the loop the production stem (384 frames x 56 rows) runs."""
    shape = (2100, 4, 4, 32)
    assert shape[0] * P.out_size(shape[1]) > 4096
    _stem_bwd(_k(), dev, shape, 91)


# ---- temporal max-pool ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('frame_elems', [32, 96, 7 * 7 * 64])
@pytest.mark.parametrize('frames_out', [1, 3, 513])
def test_temporal_pool(frame_elems, frames_out, dev):
    K = _k()
    shape = (2 * frames_out, 1, frame_elems // 32, 32)
    for name, x in (('dyadic', P.dyadic(shape, frame_elems + frames_out)),
                    ('randn', np.random.default_rng(frames_out).standard_normal(shape).astype(np.float32))):
        ref, sel = P.maxpool_t2(x)
        xd = _t(x, dev)
        _poison(dev, (ref.shape, torch.float32), ((ref.size // 32,), torch.int32))
        out, s = K.maxpool_t2_fwd(xd)
        _eq(out, ref, name + ' values')
        _eq(s, sel, name + ' sel words')
        d = P.dyadic(ref.shape, 7) if name == 'dyadic' else np.random.default_rng(8).standard_normal(ref.shape).astype(np.float32)
        d[d == 0] = 0.5                                             # so that an exact 0 in dx can only be the losing frame
        dd, seld = _t(d, dev), _t(sel, dev)
        _poison(dev, (shape, torch.float32))
        dx = K.maxpool_t2_bwd(dd, seld).cpu()
        _eq(dx, P.maxpool_t2_bwd(d, sel), name + ' dx')
        won2 = _t(P.unpack_bits(sel, ref.shape))
        assert (dx[0::2][won2] == 0).all() and (dx[1::2][~won2] == 0).all()
        assert (dx[0::2][~won2] != 0).all() and (dx[1::2][won2] != 0).all()


# ---- global average pool ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('HW', [1, 4, 49, 50])
@pytest.mark.parametrize('C', [4, 64, 2048])
def test_avgpool(HW, C, dev):
    """Forward: HW sequential fp32 additions in pixel order, one multiply by fp32(1) / fp32(HW); backward: one multiply.  No product
    feeds an addition, so there is nothing for the compiler to contract: exact."""
    K = _k()
    H, W = (7, 7) if HW == 49 else (5, 10) if HW == 50 else (HW, 1)
    for N in (1, 5):
        x = np.random.default_rng(HW + C + N).standard_normal((N, H, W, C)).astype(np.float32)
        xb = _t(x).to(BF16)
        xd, xbd = _t(x, dev), xb.to(dev)
        _poison(dev, ((N, C), torch.float32))
        _eq(K.avgpool_fwd(xd), P.avgpool(x)[1], f'fwd {x.shape}')
        _poison(dev, ((N, C), torch.float32))
        _eq(K.avgpool_fwd(xbd), P.avgpool(xb.float().numpy())[1], f'fwd bf16 {x.shape}')
        d = np.random.default_rng(C + N).standard_normal((N, C)).astype(np.float32)
        want = P.avgpool_bwd(d, HW).reshape(N, H, W, C)
        dd = _t(d, dev)
        _poison(dev, (x.shape, torch.float32))
        _eq(K.avgpool_bwd(dd, x.shape), want, f'bwd {x.shape}')
        _poison(dev, (x.shape, BF16))
        _eq(K.avgpool_bwd(dd, x.shape, BF16), _t(want).to(BF16), f'bwd bf16 {x.shape}')


# ---- relu_bwd, add ----------------------------------------------------------------------------------------------------------

def _edge_mask_words(nwords, seed):
    """Isolated set bits and isolated clear bits at the word and nibble boundaries (bits 0, 3, 4, 31), then random words."""
    single = [1 << 0, 1 << 3, 1 << 4, 1 << 31]
    pattern = single + [0xFFFFFFFF ^ b for b in single] + [0, 0xFFFFFFFF, (1 << 31) | 1, (1 << 4) | (1 << 3)]
    w = np.random.default_rng(seed).integers(0, 1 << 32, size=nwords, dtype=np.uint64).astype(np.uint32)
    k = min(nwords, len(pattern))
    w[:k] = np.array(pattern[:k], np.uint32)
    if nwords > len(pattern):
        w[-4:] = np.array(single, np.uint32)          # and in the last words of the tensor
    return w.view(np.int32)


@pytest.mark.parametrize('numel', [32, 96, 32 * 257, 32 * 8193])
def test_relu_bwd_and_add(numel, dev):
    """fp32: g = (bit ? dout : 0) [+ add], out = a + b, exactly.  bf16: the fp32 result of the widened operands, rounded once."""
    K = _k()
    rng = np.random.default_rng(numel)
    words = _edge_mask_words(numel // 32, numel)
    bits = _t(P.unpack_bits(words, (numel // 32, 32)))
    d32, a32 = (_t(rng.standard_normal((numel // 32, 32)).astype(np.float32)) for _ in range(2))
    for dt in (torch.float32, BF16):
        d, a = d32.to(dt), a32.to(dt)
        dd, ad, wd = d.to(dev), a.to(dev), _t(words, dev)
        masked = torch.where(bits, d.float(), torch.zeros(()))
        for add in (None, a):
            want = (masked if add is None else masked + a.float()).to(dt)
            what = f'relu_bwd {dt} add={add is not None}'
            _poison(dev, (d.shape, dt))
            _eq(K.relu_bwd(dd, wd, None if add is None else ad), want, what)
            buf = torch.full_like(dd, float('nan'))
            assert K.relu_bwd(dd, wd, None if add is None else ad, g=buf) is buf
            _eq(buf, want, what + ' into a supplied tensor')
        want = (d.float() + a.float()).to(dt)
        _poison(dev, (d.shape, dt))
        _eq(K.add(dd, ad), want, f'add {dt}')
        buf = torch.full_like(dd, float('nan'))
        assert K.add(dd, ad, out=buf) is buf
        _eq(buf, want, f'add {dt} into a supplied tensor')
        _eq(dd, d, 'dout untouched')
        _eq(ad, a, 'add untouched')


# ---- layout change, background mix ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (2, 3, 5, 7), (3, 3, 20, 24)])
def test_nchw3_to_nhwc4(shape, dev):
    x = torch.from_numpy(np.random.default_rng(shape[2]).standard_normal(shape).astype(np.float32))
    N, _, H, W = shape
    xd = x.to(dev)
    _poison(dev, ((N, H, W, 4), torch.float32))
    o = _k().nchw3_to_nhwc4(xd).cpu()
    _eq(o[..., :3].contiguous(), x.permute(0, 2, 3, 1).contiguous(), 'channels')
    assert (o[..., 3] == 0).all() and not torch.signbit(o[..., 3]).any()           # exactly +0


@pytest.mark.parametrize('H,W', [(5, 7), (20, 28)])
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('alpha', [0.5, 0.3])
def test_bgmix_with_a_float_background(H, W, T, alpha, dev):
    """The path bg_resize_crop_u8 feeds: an fp32 background that is not on whole grey levels.  The kernel runs without contraction,
    every operation is one rounded fp32 operation in the restatement's order: exact, in both layouts."""
    K = _k()
    B = 3
    g = torch.Generator().manual_seed(H * T)
    fr = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    bg = torch.rand(B, H, W, 3, generator=g) * 255.0
    for mix in ([1, 1, 1], [0, 0, 0], [1, 0, 1]):
        mix = torch.tensor(mix, dtype=torch.bool)
        r4, rc = O.bgmix_normalize_f32bg(fr, bg, mix, alpha)
        frd, bgd, mixd = fr.to(dev), bg.to(dev), mix.to(torch.uint8).to(dev)
        for want4, wantc in ((True, False), (False, True), (True, True)):
            _poison(dev, (r4.shape, torch.float32), (rc.shape, torch.float32))
            o4, oc = K.bgmix_normalize_u8(frd, bgd, mixd, alpha, O.IMG_MEAN, O.IMG_STD, want4, wantc)
            assert (o4 is None) == (not want4) and (oc is None) == (not wantc)
            if want4:
                _eq(o4, r4, f'NHWC4 mix {mix.tolist()}')
                assert not torch.signbit(o4.cpu()[..., 3]).any()
            if wantc:
                _eq(oc, rc, f'NCHW mix {mix.tolist()}')


# ---- dropout ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('numel', [1, 255, 257, 2048 * 256 + 5])
@pytest.mark.parametrize('seed', [0, 1234, 2 ** 63 + 5])
def test_dropout_mask_and_values(numel, seed, dev):
    """The kept set and the kept values (one fp32 multiply by the scale) against the restated generator; 2048 * 256 + 5 elements
    go past the 2048-block cap into the grid-stride loop."""
    K = _k()
    x = np.random.default_rng(numel).standard_normal(numel).astype(np.float32)
    x[x == 0] = 1.0
    xd = _t(x, dev)
    for p in (0.0, 0.5, 0.8, 0.999):
        keep, scale = P.dropout_mask(numel, p, seed)
        _poison(dev, (x.shape, torch.float32))
        out = K.dropout(xd, p, seed)
        _eq(out, np.where(keep, x * scale, np.float32(0)), f'p {p}')
        assert np.array_equal(out.cpu().numpy() != 0, keep)


@pytest.mark.parametrize('p,seed', [(0.5, 1234), (0.8, 2 ** 63 + 5)])
def test_dropout_backward_uses_the_forwards_mask(p, seed, dev):
    from bdvcil_amd import functional as Fn
    n = 32 * 257 + 3
    rng = np.random.default_rng(n)
    x, w = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    w[w == 0] = 1.0
    xt = _t(x, dev).requires_grad_(True)
    out = Fn.DropoutFn.apply(xt, p, seed)
    (out * _t(w, dev)).sum().backward()
    keep, scale = P.dropout_mask(n, p, seed)
    _eq(out.detach(), np.where(keep, x * scale, np.float32(0)), 'forward')
    _eq(xt.grad, np.where(keep, w * scale, np.float32(0)), 'gradient')
