"""The 'f16x2' conv arithmetic, restated in torch on the CPU: the definition the GPU tests (tests/test_f16x2_gpu.py) use.

An operand tensor t gets the power-of-two scale S_t = 2^(14 - floor(log2 max|t|)) (exponent clamped to [-113, 126]; 1 for a zero
tensor), so that max|t| * S_t lies in [2^14, 2^15); x = t * S_t is cut into hi = f16(x) and lo = f16(x - hi), round to nearest even;
a product a * w is hi_a * hi_w + hi_a * lo_w + lo_a * hi_w, and the sum is multiplied by 1 / (S_a * S_w) (exponent clamped to the
normal fp32 range).  Here the three products are accumulated in fp64, so what is measured is the split alone."""
import math

import pytest
import torch


def f16x2_scale(t: torch.Tensor) -> float:
    """S_t of a tensor, from its maximum."""
    m = float(t.detach().abs().max()) if t.numel() else 0.0
    if m == 0.0:
        return 1.0
    if math.isinf(m) or math.isnan(m):
        return 2.0 ** -113
    e = 14 - (math.frexp(m)[1] - 1)          # frexp: m = f * 2^ex with f in [0.5, 1)  ->  floor(log2 m) = ex - 1
    return 2.0 ** max(-113, min(126, e))


def f16x2_unscale(sa: float, sw: float) -> float:
    """1 / (S_a * S_w) with the exponent clamped to the normal fp32 range."""
    e = -(math.frexp(sa)[1] - 1) - (math.frexp(sw)[1] - 1)
    return 2.0 ** max(-126, min(127, e))


def f16x2_split(t: torch.Tensor, scale: float):
    """(hi, lo) as fp64 tensors holding fp16 values."""
    x = (t.float() * scale).float()          # a power of two: exact unless it leaves fp32's range
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


def f16x2_matmul(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """a (M, K) @ w (K, N) in the arithmetic, products accumulated in fp64."""
    sa, sw = f16x2_scale(a), f16x2_scale(w)
    (ah, al), (wh, wl) = f16x2_split(a, sa), f16x2_split(w, sw)
    return (al @ wh + ah @ wl + ah @ wh) * f16x2_unscale(sa, sw)


def _lib_scale(m: float) -> float:
    import bdvcil_amd as bd
    return float(bd._lib.lib().bdv_f16x2_scale(m))


def test_scale_of_a_zero_tensor_is_one():
    assert f16x2_scale(torch.zeros(7)) == 1.0
    assert _lib_scale(0.0) == 1.0
    hi, lo = f16x2_split(torch.zeros(7), 1.0)
    assert not hi.any() and not lo.any()


@pytest.mark.parametrize('m', [1e-30, 1e30, 65504.0, 3.4028234663852886e38, 1.0, 2.0 ** -20, 2.0 ** 40, 2.0 ** -112, 3.0, 0.75])
def test_scaled_maximum_lies_in_the_top_fp16_binade(m):
    t = torch.tensor([m, -m / 3, 0.0], dtype=torch.float32)
    m32 = float(t.abs().max())
    s = f16x2_scale(t)
    assert s == _lib_scale(m32)                                   # the library's rule is this rule
    assert s == 2.0 ** round(math.log2(s)) and 2.0 ** -126 <= s <= 2.0 ** 127        # a normal fp32 power of two
    assert 2.0 ** 14 <= m32 * s < 2.0 ** 15
    hi, lo = f16x2_split(t, s)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert float((hi + lo)[0]) / s == pytest.approx(m32, rel=2.0 ** -21)
    if m32 == 2.0 ** round(math.log2(m32)):                        # an exact power of two lands on 2^14 itself
        assert m32 * s == 2.0 ** 14 and float(hi[0]) == 2.0 ** 14 and float(lo[0]) == 0.0


def test_maxima_outside_the_scalable_range_keep_a_normal_scale():
    """Below 2^-112 the exponent is clamped: the scale stays the largest normal power of two that is allowed, the scaled maximum
    falls short of 2^14 (bits are lost, nothing overflows).  Inf / NaN take the smallest scale and propagate."""
    for m in (2.0 ** -120, 1e-40):
        t = torch.tensor([m], dtype=torch.float32)
        s = f16x2_scale(t)
        assert s == 2.0 ** 126 == _lib_scale(float(t[0]))
        assert float(t[0]) * s < 2.0 ** 14
    assert _lib_scale(float('inf')) == 2.0 ** -113 == f16x2_scale(torch.tensor([float('inf')]))
    hi, lo = f16x2_split(torch.tensor([float('inf'), 1.0]), 2.0 ** -113)
    assert torch.isinf(hi[0]) and torch.isnan(lo[0])


def test_unscale_stays_normal():
    for sa, sw in ((2.0 ** 126, 2.0 ** 126), (2.0 ** -113, 2.0 ** -113), (2.0 ** 51, 2.0 ** -28), (1.0, 1.0)):
        u = f16x2_unscale(sa, sw)
        assert 2.0 ** -126 <= u <= 2.0 ** 127
        if 2.0 ** -126 <= 1.0 / (sa * sw) <= 2.0 ** 127:
            assert u == 1.0 / (sa * sw)


def test_three_products_reach_fp32_level():
    """Post-ReLU activations x kaiming weights, 2048 x 2304 x 256: the error of the split (max error as a fraction of max|C|,
    against fp64) stays within 4 x the error of the fp32 CPU matmul of the same operands (measured 0.26 x of an fp32 FMA chain; the
    margin covers other seeds and a blocked matmul's smaller error)."""
    gen = torch.Generator().manual_seed(0)
    a = torch.randn(2048, 2304, generator=gen).clamp_min(0)
    w = torch.randn(2304, 256, generator=gen) * math.sqrt(2.0 / 2304)
    c64 = a.double() @ w.double()
    scale = float(c64.abs().max())
    e32 = float(((a @ w).double() - c64).abs().max()) / scale
    e16 = float((f16x2_matmul(a, w) - c64).abs().max()) / scale
    print(f'[f16x2 emulation] max error / max|C|: f16x2 {e16:.2e}, fp32 matmul {e32:.2e}')
    assert e16 <= 4 * e32, (e16, e32)
    # and it is far from the two-bf16-piece arithmetic it stands beside (16 significand bits per operand)
    ah = a.to(torch.bfloat16).float()
    am = (a - ah).to(torch.bfloat16).float()
    wh = w.to(torch.bfloat16).float()
    wm = (w - wh).to(torch.bfloat16).float()
    eb = float(((am.double() @ wh.double() + ah.double() @ wm.double() + ah.double() @ wh.double()) - c64).abs().max()) / scale
    assert eb >= 10 * e16, (eb, e16)


def test_set_conv_arith_knows_the_mode():
    from bdvcil_amd import kernels as K
    prev = K.set_conv_arith('f16x2')
    try:
        assert K.PIECES == K.F16X2 == 4 and K.ACT_DTYPE == torch.float32
        assert (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3) == (True, True, True)
    finally:
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev
    assert K.PIECES == 3


# (N, H, W, Cin, Cout, R, stride, pad, T, fold) -> (fprop, dgrad, wgrad): does the direction run the two-fp16-piece kernel?
PLAN_CASES = [
    ((8, 14, 14, 64, 128, 1, 1, 0, 8, 8), (True, False, False)),     # dgrad: 64 columns behind 1x1; wgrad: no plane tile for 64 -> 128
    ((8, 14, 14, 128, 128, 3, 1, 1, 8, 0), (True, True, True)),
    ((8, 28, 28, 128, 128, 3, 2, 1, 8, 0), (True, True, True)),
    ((16, 7, 7, 256, 512, 1, 1, 0, 8, 32), (True, True, True)),
    ((8, 14, 14, 256, 64, 1, 1, 0, 8, 32), (False, True, True)),     # fprop: 64 columns behind 1x1
    ((8, 14, 14, 64, 64, 3, 1, 1, 8, 0), (True, True, True)),
]


@pytest.mark.parametrize('case,f16', PLAN_CASES)
def test_plan_names_the_fp16_kernels_and_keeps_the_other_arithmetics(case, f16):
    """The plan query needs no GPU: arith 4 gives the F16Pieces kernels at the plane-kernel sites and the three-bf16-piece plan
    elsewhere; the plans of the existing arithmetics do not move (tests/test_conv_plan_cpu.py holds them to the golden file)."""
    from bdvcil_amd import kernels as K
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold)
    prev = K.set_conv_arith('bf16x3')
    try:
        x3 = [K.conv_plan(g, k) for k in ('fprop', 'dgrad', 'wgrad')]
        x3 = [(p.kernel.decode(), p.family, p.stat_rows, p.splits) for p in x3]
        K.set_conv_arith('bf16x2')
        x2 = [K.conv_plan(g, k) for k in ('fprop', 'dgrad', 'wgrad')]
        x2 = [(p.kernel.decode(), p.family, p.stat_rows, p.splits) for p in x2]
        K.set_conv_arith('f16x2')
        for i, kind in enumerate(('fprop', 'dgrad', 'wgrad')):
            p = K.conv_plan(g, kind)
            got = (p.kernel.decode(), p.family, p.stat_rows, p.splits)
            if f16[i]:
                assert got[0].endswith('F16Pieces>') and f'conv_{kind}_pl_kernel<' in got[0], got
                assert got[1:] == x2[i][1:], (got, x2[i])          # the tile (hence the side buffers) of the two-piece rules
            else:
                assert got == x3[i], (got, x3[i])
    finally:
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev


def test_stem_and_loader_batchnorm_keep_three_bf16_pieces():
    from bdvcil_amd import kernels as K
    stem = K.make_geom(8, 32, 32, 4, 64, 7, 7, 2, 3)
    site = K.make_geom(8, 14, 14, 128, 128, 3, 3, 1, 1)
    prev = K.set_conv_arith('bf16x3')
    try:
        want = [K.conv_plan(stem, 'fprop').kernel, K.conv_plan(stem, 'wgrad').kernel, K.conv_plan(site, 'fprop', pre=True).kernel]
        K.set_conv_arith('f16x2')
        got = [K.conv_plan(stem, 'fprop').kernel, K.conv_plan(stem, 'wgrad').kernel, K.conv_plan(site, 'fprop', pre=True).kernel]
        assert got == want
        assert not K.fprop_pre_ok(site)
    finally:
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev
