"""Edge sweep of the heads in csrc/head_loss.hip -- head_fwd_kernel (LSC and linear), lsc_bwd_dx / lsc_bwd_dw, linear_bwd_dx /
linear_bwd_dw, consensus and dropout -- and of LSCFn / LinearFn / ConsensusFn / DropoutFn around them, against the fp64 run of
oracle/step_tail_oracle.py (held against the reference's goldens in tests/test_step_tail_cpu.py), never against a sibling kernel.
Sizes reach what the one-shape tests of test_ops_gpu.py do not: N off the 4 rows a block stages, D below 64 and off the 64 / 256
strides, K * P off the 4 waves and above 256, K off the 8 classes of a linear_bwd_dw block, D + K * P = 3750 and N = 1875 (the LDS
limits exactly), and the first size past each limit, which the entry points refuse before any launch.

Bars
  * exact: zeros, NaN positions, refusals, dropout masks and kept values, consensus on a dyadic grid (multiples of 1/8, T in {1, 8})
    and its backward for any input when T is a power of two, everything a second path must reproduce bit for bit (need_dw=False,
    need_dx=False, beta_w = 0 onto NaN, the autograd functions over the same kernels);
  * sim, xnorm, wnorm, cosbuf, dx, dw, db, consensus at T = 3: floor * max(1, scale) + 4 x the largest deviation of the fp32 CPU oracle
    from the fp64 oracle on the same case (from the two references only), floor 2e-7 for the linear head's plain dot products, 2e-6 for
    everything through a division, sqrtf or expf; never looser than test_ops_gpu.py's bar for the quantity (1e-5 * scale + 1e-6
    forward and linear gradients, 1e-4 * scale + 1e-7 LSC gradients);
  * beta_w = 1 onto a prior dw / db: that bar plus one rounding of the sum, 2^-24 * (|prior| + |gradient|) per element;
  * dropout keep rate at n = 2^20: 5 * sqrt(p (1 - p) / n).

Largest error / bar observed on an MI355X (recorded per test with record_property):
  LSC: sim 0.023 ((2, 65, 300, 2)), xnorm 0.028, wnorm 0.045 ((4, 2048, 851, 2)), cosbuf 0.038, dx 0.075 and dw 0.030
  ((2, 65, 300, 2)), dw onto a prior dw 0.031; linear: out 0.189 ((4, 64, 8)), dx 0.186 ((2, 65, 300)), dw 0.172, db 0.160, onto a
  prior dw / db 0.280 ((7, 2048, 101)), dw of the 1875-row sum 0.100; consensus at T = 3 0.034 (its backward 0.015); dropout keep
  rate 0.237 (p = 0.8);
  everything else is exact.

Found by this file: LSC (1, 1, 1, 1) backward stood at dx 1.469 and dw 1.144 of its bar.  With D = 1 the cosine is +-1 whatever x and
  w are, the reference gradient is 0 exactly and the bar is the bare 1e-7 of test_ops_gpu.py's gradient tolerance.  lsc_bwd_dx /
  lsc_bwd_dw formed the gradient as sum_j G_j w_j - a_n x_n, two sums of size |dsim / x| = 1.28 rounded apart, and left an ulp of
  them (the same loss of digits whenever the features lie along their proxies).  They now subtract from every row its own
  component, sum_j G_j (w_j - cos_j |w_j| x / |x|): dx and dw of the case are 0 exactly, the other cases moved by less than 0.03
  of their bars (dx of (2, 65, 300, 2) from 0.052 to 0.075).

Outputs are allocated inside the wrappers; ``_poison`` (see test_pool_kernels_gpu.py) is a best effort against stale correct
values and nothing rests on it.
"""
import numpy as np
import pytest
import torch

from oracle import step_tail_oracle as S

pytestmark = pytest.mark.gpu

U = S.U


def _k():
    from bdvcil_amd import kernels as K
    return K


def _poison(dev, *tensors_like):
    blocks = [torch.full((max(1, int(np.prod(shape))) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev)
              for shape, dtype in tensors_like]
    torch.cuda.synchronize()
    del blocks


def _ratio(got, ref64, bar):
    """Largest |got - ref| / bar (bar: a float or a tensor of ref's shape); shapes and NaN positions must agree."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), 'NaN positions differ'
    err = torch.nan_to_num((got - ref64).abs(), nan=0.0)
    return (err / bar).max().item() if err.numel() else 0.0


def _check(what, got, ref64, bars, record_property, defer=False):
    """Every named quantity within its bar; prints and records each ratio before asserting (``defer``: the caller asserts, after the
    checks that do not depend on these)."""
    ratios = {k: _ratio(got[k], ref64[k], bars[k]) for k in got}
    print(f'{what}: ' + ', '.join(f'{k} {r:.3f} (bar {bars[k]:.2e})' for k, r in ratios.items()))
    for k, r in ratios.items():
        record_property(f'{k} err/bar', r)
    assert defer or all(r <= 1.0 for r in ratios.values()), (what, ratios)
    return ratios


# ---- LSC -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ci', range(len(S.LSC_CASES)))
def test_lsc_ragged(ci, dev, record_property):
    from bdvcil_amd import functional as Fn
    K_ = _k()
    N, D, K, P = S.LSC_CASES[ci]
    (x, w, dsim, _, _), r64, bars = S.lsc_case(ci)
    xd, wd, gd = x.to(dev), w.to(dev), dsim.to(dev)
    _poison(dev, ((N, K), torch.float32), ((N,), torch.float32), ((K * P,), torch.float32), ((N, K * P), torch.float32))
    sim, xn, wn, cb = K_.lsc_fwd(xd, wd, K, P)
    _poison(dev, ((N, D), torch.float32), ((K, P * D), torch.float32))
    dx, dw = K_.lsc_bwd(gd, xd, wd, xn, wn, cb, K, P)
    ratios = _check(f'lsc {S.LSC_CASES[ci]}', dict(sim=sim, xnorm=xn, wnorm=wn, cosbuf=cb, dx=dx, dw=dw), r64, bars, record_property, defer=True)
    # need_dw=False: the dx pass alone
    dx2, none = K_.lsc_bwd(gd, xd, wd, xn, wn, cb, K, P, need_dw=False)
    assert none is None and torch.equal(dx2, dx)
    # beta_w = 1 onto a prior dw; beta_w = 0 onto NaN
    prior = torch.randn(K, P * D, generator=torch.Generator().manual_seed(3200 + ci)) * r64['dw'].abs().max().float()
    acc = prior.to(dev)
    _, out = K_.lsc_bwd(gd, xd, wd, xn, wn, cb, K, P, dw=acc, beta_w=1.0)
    assert out is acc
    want = prior.double() + r64['dw']
    r_acc = _ratio(acc, want, bars['dw'] + U * (prior.double().abs() + r64['dw'].abs()))
    print(f'lsc {S.LSC_CASES[ci]}: dw onto a prior dw {r_acc:.3f}')
    record_property('dw accumulated err/bar', r_acc)
    nan = torch.full((K, P * D), float('nan'), device=dev)
    K_.lsc_bwd(gd, xd, wd, xn, wn, cb, K, P, dw=nan, beta_w=0.0)
    assert torch.equal(nan, dw)                                              # no NaN left, and the same values
    # LSCFn: the same kernels behind autograd, with and without a weight gradient
    xa, wa = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    sa = Fn.LSCFn.apply(xa, wa, K, P)
    sa.backward(gd)
    assert torch.equal(sa.detach(), sim) and torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw)
    xb = xd.clone().requires_grad_(True)
    Fn.LSCFn.apply(xb, wd, K, P).backward(gd)
    assert torch.equal(xb.grad, dx)
    assert all(r <= 1.0 for r in ratios.values()) and r_acc <= 1.0, (S.LSC_CASES[ci], ratios, r_acc)


def test_lsc_zero_rows(dev, record_property):
    """A zero row of x: sim is 0 exactly (0 / (eps * |w|)), its norm is the eps clamp, the other rows do not notice.  Forward only:
    the backward there is defined by the clamp and is not asserted."""
    ci = 3
    N, D, K, P = S.LSC_CASES[ci]
    x, w, _, _, _ = S.head_input('lsc', ci)
    x = x.clone()
    x[1] = 0.0
    x[4] = 0.0                                                               # the one row of the second block
    r64, r32 = S.lsc_head(x.double(), w.double(), K, P), S.lsc_head(x, w, K, P)
    bars = {k: S.bar(r64[k], r32[k], S.FLOOR_FN, S.CAP_FWD) for k in r64}
    sim, xn, wn, cb = _k().lsc_fwd(x.to(dev), w.to(dev), K, P)
    for rows in (1, 4):
        assert torch.equal(sim[rows].cpu(), torch.zeros(K)) and torch.equal(cb[rows].cpu(), torch.zeros(K * P))
        assert torch.equal(r64['sim'][rows], torch.zeros(K, dtype=torch.float64))
        assert xn[rows].item() == S.f32(S.COS_EPS)
    assert torch.isfinite(sim).all()
    _check('lsc zero rows', dict(sim=sim, xnorm=xn, wnorm=wn, cosbuf=cb), r64, bars, record_property)


# ---- linear --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('ci', range(len(S.LINEAR_CASES)))
def test_linear_ragged(ci, with_bias, dev, record_property):
    from bdvcil_amd import functional as Fn
    K_ = _k()
    N, D, K = S.LINEAR_CASES[ci]
    (x, w, b, dout), r64, bars = S.linear_case(ci, with_bias)
    xd, wd, gd = x.to(dev), w.to(dev), dout.to(dev)
    bd_ = None if b is None else b.to(dev)
    _poison(dev, ((N, K), torch.float32))
    out = K_.linear_fwd(xd, wd, bd_)
    _poison(dev, ((N, D), torch.float32), ((K, D), torch.float32), ((K,), torch.float32))
    dx, dw, db = K_.linear_bwd(gd, xd, wd, need_db=with_bias)
    got = dict(out=out, dx=dx, dw=dw)
    if with_bias:
        got['db'] = db
    else:
        assert db is None
    _check(f'linear {S.LINEAR_CASES[ci]} bias={with_bias}', got, r64, bars, record_property)
    # need_dx=False: the weight pass alone
    none, dw2, db2 = K_.linear_bwd(gd, xd, wd, need_dx=False, need_db=with_bias)
    assert none is None and torch.equal(dw2, dw) and (not with_bias or torch.equal(db2, db))
    # beta_w = 1 onto a prior dw / db; beta_w = 0 onto NaN
    g = torch.Generator().manual_seed(3300 + ci)
    prior_w = torch.randn(K, D, generator=g) * r64['dw'].abs().max().float()
    acc_w = prior_w.to(dev)
    prior_b = acc_b = None
    if with_bias:
        prior_b = torch.randn(K, generator=g) * r64['db'].abs().max().float()
        acc_b = prior_b.to(dev)
    K_.linear_bwd(gd, xd, wd, need_dx=False, dw=acc_w, db=acc_b, beta_w=1.0)
    r_acc = _ratio(acc_w, prior_w.double() + r64['dw'], bars['dw'] + U * (prior_w.double().abs() + r64['dw'].abs()))
    if with_bias:
        r_acc = max(r_acc, _ratio(acc_b, prior_b.double() + r64['db'], bars['db'] + U * (prior_b.double().abs() + r64['db'].abs())))
    print(f'linear {S.LINEAR_CASES[ci]} bias={with_bias}: dw / db onto a prior value {r_acc:.3f}')
    record_property('accumulated err/bar', r_acc)
    assert r_acc <= 1.0
    nan_w = torch.full((K, D), float('nan'), device=dev)
    nan_b = torch.full((K,), float('nan'), device=dev) if with_bias else None
    K_.linear_bwd(gd, xd, wd, need_dx=False, dw=nan_w, db=nan_b, beta_w=0.0)
    assert torch.equal(nan_w, dw) and (not with_bias or torch.equal(nan_b, db))
    # LinearFn: the same kernels behind autograd; an input that needs no gradient
    xa, wa = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    ba = None if bd_ is None else bd_.clone().requires_grad_(True)
    oa = Fn.LinearFn.apply(xa, wa, ba)
    oa.backward(gd)
    assert torch.equal(oa.detach(), out) and torch.equal(xa.grad, dx) and torch.equal(wa.grad, dw)
    assert not with_bias or torch.equal(ba.grad, db)
    wb = wd.clone().requires_grad_(True)
    Fn.LinearFn.apply(xd, wb, bd_).backward(gd)
    assert torch.equal(wb.grad, dw)


# ---- refusals: each call fails on its sizes before any launch -------------------------------------------------------------------

def test_lds_limits_are_refused(dev):
    import bdvcil_amd as bd
    K_ = _k()
    err = bd._lib.HipExtensionError
    z = lambda *shape: torch.zeros(*shape, device=dev)                      # noqa: E731
    with pytest.raises(err, match=r'bdv_lsc_fwd: D \+ K\*P too large for LDS'):
        K_.lsc_fwd(z(1, 2049), z(851, 2 * 2049), 851, 2)                     # 4 * (2049 + 1702) * 4 = 60016 bytes
    N = 15001
    with pytest.raises(err, match='bdv_lsc_bwd: N or K\\*P too large for LDS'):
        K_.lsc_bwd(z(N, 1), z(N, 1), z(1, 1), z(N), z(1), z(N, 1), 1, 1)
    with pytest.raises(err, match='bdv_lsc_bwd: N or K\\*P too large for LDS'):
        K_.lsc_bwd(z(1, 15001), z(1, 1), z(15001, 1), z(1), z(15001), z(1, 15001), 15001, 1)
    N = 1876
    with pytest.raises(err, match='bdv_linear_bwd: N or K too large for LDS'):
        K_.linear_bwd(z(N, 3), z(N, 5), z(3, 5))
    with pytest.raises(err, match='bdv_linear_fwd: D \\+ K too large for LDS'):
        K_.linear_fwd(z(1, 3750), z(1, 3750), None)                          # 4 * 3751 * 4 bytes


# ---- consensus -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', range(len(S.CONSENSUS_CASES)))
def test_consensus_ragged(case, dev, record_property):
    from bdvcil_amd import functional as Fn
    K_ = _k()
    B, T, Kc = S.CONSENSUS_CASES[case]
    g = torch.Generator().manual_seed(3400 + case)
    pow2 = T & (T - 1) == 0
    s = S.dyadic((B * T, Kc), g) if pow2 else torch.randn(B * T, Kc, generator=g)
    d = torch.randn(B, Kc, generator=g)
    ref, dref = S.consensus(s.double(), B, T), S.consensus_grad(d.double(), T)
    _poison(dev, ((B, Kc), torch.float32))
    out = K_.consensus_fwd(s.to(dev), B, T)
    _poison(dev, ((B * T, Kc), torch.float32))
    ds = K_.consensus_bwd(d.to(dev), T)
    assert out.shape == (B, Kc) and ds.shape == (B * T, Kc)
    if pow2:
        assert torch.equal(out.cpu().double(), ref) and torch.equal(ds.cpu().double(), dref)
    else:
        bars = dict(out=S.bar(ref, S.consensus(s, B, T), S.FLOOR_FN, S.CAP_FWD),
                    ds=S.bar(dref, S.consensus_grad(d, T), S.FLOOR_FN, S.CAP_FWD))
        _check(f'consensus {S.CONSENSUS_CASES[case]}', dict(out=out, ds=ds), dict(out=ref, ds=dref), bars, record_property)
    sa = s.to(dev).view(B, T, Kc).requires_grad_(True)
    oa = Fn.ConsensusFn.apply(sa)
    oa.backward(d.to(dev).view(B, 1, Kc))
    assert oa.shape == (B, 1, Kc) and torch.equal(oa.detach().view(B, Kc), out) and torch.equal(sa.grad.view(B * T, Kc), ds)


# ---- dropout -------------------------------------------------------------------------------------------------------------

DROPOUT_N = [1, 255, 257, 524288 + 3]           # the last one is past one grid pass of 2048 blocks of 256


def _scale(p):
    return (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)))


@pytest.mark.parametrize('p', [0.5, 0.8, 0.3])
def test_dropout_is_a_function_of_seed_and_index(p, dev):
    K_ = _k()
    n_full = DROPOUT_N[-1]
    x = torch.rand(n_full, generator=torch.Generator().manual_seed(3500)) + 0.5      # no zeros: a zero output is a dropped element
    xd = x.to(dev)
    _poison(dev, ((n_full,), torch.float32))
    full = K_.dropout(xd, p, 77)
    keep = full != 0
    assert torch.equal(full.cpu(), torch.where(keep.cpu(), x * _scale(p), torch.zeros(())))     # kept values: x * 1/(1-p) in fp32
    assert 0 < int(keep.sum()) < n_full
    for n in DROPOUT_N:
        assert torch.equal(K_.dropout(xd[:n].contiguous(), p, 77), full[:n]), n
    assert not torch.equal(K_.dropout(xd, p, 78) != 0, keep)
    assert torch.equal(K_.dropout(xd, 0.0, 77), xd)                                    # p = 0: the identity


@pytest.mark.parametrize('p', [0.5, 0.8])
def test_dropout_keep_rate_and_backward_mask(p, dev, record_property):
    from bdvcil_amd import functional as Fn
    n = 1 << 20
    x = (torch.rand(n, generator=torch.Generator().manual_seed(3501)) + 0.5).to(dev).requires_grad_(True)
    y = Fn.DropoutFn.apply(x, p, 1234)
    keep = y.detach() != 0
    rate = keep.float().mean().item()
    bound = 5 * (p * (1 - p) / n) ** 0.5
    print(f'dropout p={p}: keep rate {rate:.6f}, |rate - (1 - p)| / bound {abs(rate - (1 - p)) / bound:.3f}')
    record_property('keep rate err/bar', abs(rate - (1 - p)) / bound)
    assert abs(rate - (1 - p)) <= bound
    up = torch.rand(n, generator=torch.Generator().manual_seed(3502)) + 0.5
    y.backward(up.to(dev))
    assert torch.equal(x.grad.cpu(), torch.where(keep.cpu(), up * _scale(p), torch.zeros(())))   # the forward mask, the same scale
