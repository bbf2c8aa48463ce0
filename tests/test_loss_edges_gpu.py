"""Edge sweep of the loss kernels in csrc/head_loss.hip -- lsc_loss_kernel, softce_kernel, icarl_targets_kernel, acm_targets_kernel,
sqdiff_partial / mse_finalize / kd_mse_bwd (fp32 and bf16 storage) -- and of LSCLossFn / SoftCEFn / KDMSEFn around them, against the
fp64 run of oracle/step_tail_oracle.py (held against the reference's goldens in tests/test_step_tail_cpu.py), never against a sibling
kernel.  (B, K) runs from (1, 1) over B off the 4 waves and K on and off the 64 lanes to K = 300 and B = 130; the KD sizes sit on
both sides of a block and of the 4 * 256 * 1024 elements of one grid pass.

Bars
  * exact: (1, 1) gives loss 0, dsim 0, deta 0; one-hot, copied and ``base`` target rows; fg_ratio 0 and 1; refusals; an upstream
    gradient of 0.25 scales the saved gradients bit for bit;
  * an LSCLoss case is the first of 20 seeds whose fp64 run decides every row's arg-max by 1e-4, and with the hinge on every row's
    value by 1e-4, so that fp32 cannot flip either; with a negative class weight there is a row on either side of zero.  A single
    class gives every row the value 0 exactly in any precision, and one row cannot be on both sides: (1, 1) is exempt from the last
    two conditions.  No case is dropped (tests/test_step_tail_cpu.py);
  * loss, dsim, deta, dscore, softmax and ActorCutMix target rows: 2e-6 * max(1, scale) + 4 x the largest deviation of the fp32 CPU
    oracle from the fp64 oracle on the same case (from the two references only), never looser than test_ops_gpu.py's bar for the
    quantity (loss 1e-5 * scale + 1e-6, dsim / deta 1e-4 * scale + 1e-7, dscore and softmax rows 1e-5 * scale + 1e-7, ActorCutMix
    rows, and iCaRL targets over ActorCutMix base rows, 1e-6 * scale + 1e-6);
  * kd_mse forward: 32 * 2^-24 relative (non-negative terms: at most 12 per thread, a 6-level wave tree, 4 waves, an fp64 finalize);
    backward, per element: 5 * 2^-24 * |ref| (four roundings, no sum; tighter than the general rule, which is void at a gradient of
    1e-6), plus half a bf16 ulp of the value for the bf16 gradient.  bf16 inputs are exact in fp64.

LSCLoss seeds: 20000 + 100 * case + t; every case takes t = 0 except
  (5, 65) eta 1 margin 0.6 hinge off positive 1; (6, 101) eta 1 margin 0 hinge on positive 1; (9, 300) eta 0.37: margin 0 hinge off
  positive 1, hinge on none 1, negative 2, margin 0.6 positive 1 (hinge off and on); (9, 300) eta 1: margin 0 hinge on positive 1,
  margin 0.6 hinge on none 1; (130, 37) eta 0.37: margin 0 hinge off positive 1, margin 0.6 hinge off none 1, hinge on none 2,
  positive 1, negative 3; (130, 37) eta 1: margin 0 hinge off positive 1, hinge on none 1, margin 0.6 hinge off negative 4
  (tests/test_step_tail_cpu.py prints the list).

Largest error / bar observed on an MI355X (recorded per test with record_property):
  lsc_loss: loss 0.084, dsim 0.069 (both (3, 5), hinge off, one negative weight), deta 0.042; softce: loss 0.680 ((1, 1), rows summing
  to 0.7), dscore 0.456 ((4, 64), ActorCutMix rows, logits of +-80); icarl_targets 0.056, acm_targets 0.026 (both (130, 37));
  kd_mse forward 0.035, backward 0.615 of the fp32 bar; the bf16 gradient 1.000 (1024 elements) and 0.996 through KDMSEFn: the
  kernel rounds to nearest, so half an ulp is reached and the fp32 part of the bar is what is left over.

Found by this file: with one class, lsc_loss_kernel returned a loss of -7.8e-9 to 5.5e-9 where the reference gives 0 exactly (six of six
  (1, 1) cases failed the exact bar).  "eta * (sim - margin) - mx" was compiled into one fused multiply-add, whose value at the
  arg-max is the rounding error of the product instead of 0 -- in every row of every shape, where it only moves the largest term
  from exp(0) to exp(1e-9).  The product is now rounded on its own (lsc_logit): loss, dsim and deta at (1, 1) are 0 exactly.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import step_tail_oracle as S

pytestmark = pytest.mark.gpu


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


# ---- LSCLoss -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('wkind', S.WEIGHTS)
@pytest.mark.parametrize('hinge', [False, True])
@pytest.mark.parametrize('bi', range(len(S.LOSS_BK)))
def test_lsc_loss_edges(bi, hinge, wkind, dev, record_property):
    from bdvcil_amd import functional as Fn
    K_ = _k()
    B, K = S.LOSS_BK[bi]
    worst = dict(loss=0.0, dsim=0.0, deta=0.0)
    seeds = {}
    for case, spec in enumerate(S.LSC_LOSS_CASES):
        if (spec[0], spec[3], spec[4]) != (bi, hinge, wkind):
            continue
        _, eta, margin, _, _ = spec
        (sim, targets, eta_t, cw), t, r64, bars = S.lsc_loss_case(case)
        seeds[(eta, margin)] = t
        sd, yd, ed = sim.to(dev), targets.to(dev), eta_t.to(dev)
        cd = None if cw is None else cw.to(dev)
        _poison(dev, ((2,), torch.float32), ((B, K), torch.float32))
        loss, dsim, deta = K_.lsc_loss(sd, yd, ed, margin, hinge, cd)
        assert loss.shape == () and dsim.shape == (B, K) and deta.shape == (1,)
        got = dict(loss=loss, dsim=dsim, deta=deta)
        ratios = {k: _ratio(got[k].reshape(r64[k].shape), r64[k], bars[k]) for k in got}
        print(f'lsc_loss {(B, K)} eta={eta} margin={margin} hinge={hinge} weights={wkind} t={t}: '
              + ', '.join(f'{k} {r:.3f}' for k, r in ratios.items()))
        for k, r in ratios.items():
            worst[k] = max(worst[k], r)
        if K == 1:                                            # one class: log(1) - 0, and -1 + 1/den at the arg-max
            assert loss.item() == 0 and not dsim.any() and not deta.any()
        # LSCLossFn: an upstream gradient of 0.25 scales the saved gradients
        sa, ea = sd.clone().requires_grad_(True), ed.clone().requires_grad_(True)
        la = Fn.LSCLossFn.apply(sa, yd, ea, margin, hinge, cd)
        la.backward(torch.tensor(0.25, device=dev))
        assert torch.equal(la.detach(), loss) and torch.equal(sa.grad, dsim * 0.25) and torch.equal(ea.grad, deta * 0.25)
    assert len(seeds) == len(S.ETAS) * len(S.LOSS_MARGINS)
    record_property('t', str(seeds))
    for k, r in worst.items():
        record_property(f'lsc_loss {k} err/bar', r)
    assert all(r <= 1.0 for r in worst.values()), worst


# ---- soft / plain cross entropy ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', S.SOFT_KINDS)
@pytest.mark.parametrize('bi', range(len(S.LOSS_BK)))
def test_softce_edges(bi, kind, dev, record_property):
    from bdvcil_amd import functional as Fn
    K_ = _k()
    B, K = S.LOSS_BK[bi]
    worst = dict(loss=0.0, dscore=0.0)
    for scale in S.SCORE_SCALES:
        (score, soft, labels), r64, bars = S.softce_case(bi, kind, scale)
        sd = score.to(dev)
        td = None if soft is None else soft.to(dev)
        yd = None if labels is None else labels.to(dev)
        _poison(dev, ((1,), torch.float32), ((B, K), torch.float32))
        loss, dscore = K_.softce_loss(sd, soft_targets=td, labels=yd)
        assert loss.shape == () and dscore.shape == (B, K) and torch.isfinite(loss) and torch.isfinite(dscore).all()
        got = dict(loss=loss, dscore=dscore)
        ratios = {k: _ratio(got[k], r64[k], bars[k]) for k in got}
        print(f'softce {(B, K)} {kind} x{scale:g}: ' + ', '.join(f'{k} {r:.3f} (bar {bars[k]:.2e})' for k, r in ratios.items()))
        for k, r in ratios.items():
            worst[k] = max(worst[k], r)
        sa = sd.clone().requires_grad_(True)
        la = Fn.SoftCEFn.apply(sa, td, yd)
        la.backward(torch.tensor(0.25, device=dev))
        assert torch.equal(la.detach(), loss) and torch.equal(sa.grad, dscore * 0.25)
    for k, r in worst.items():
        record_property(f'softce {k} err/bar', r)
    assert all(r <= 1.0 for r in worst.values()), worst


# ---- target builders -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bi', range(len(S.LOSS_BK)))
def test_icarl_targets_edges(bi, dev, record_property):
    K_ = _k()
    B, K = S.LOSS_BK[bi]
    g = torch.Generator().manual_seed(23000 + bi)
    labels = torch.randint(0, K, (B,), generator=g)
    prev = torch.randn(B, K, generator=g) * 3
    base = S.acm_targets(labels, torch.randint(-1, K, (B,), generator=g), torch.rand(B, generator=g), 4.0, K)
    worst = 0.0
    for prev_K in sorted({0, K // 2, K}):
        for use_prev in (True, False):
            for use_base in (False, True):
                pl, bs = (prev if use_prev else None), (base if use_base else None)
                ref = S.icarl_targets(labels, K, None if pl is None else pl.double(), prev_K, None if bs is None else bs.double())
                ref32 = S.icarl_targets(labels, K, pl, prev_K, bs)
                b = S.bar(ref, ref32, S.FLOOR_FN, *((S.CAP_GRAD5, S.CAP_TGT) if use_base else (S.CAP_GRAD5,)))   # test_ops_gpu.py's two bars
                _poison(dev, ((B, K), torch.float32))
                tgt = K_.icarl_targets(labels.to(dev), None if pl is None else pl.to(dev), prev_K, K, None if bs is None else bs.to(dev))
                assert tgt.shape == (B, K) and tgt.dtype == torch.float32
                r = _ratio(tgt, ref, b)
                worst = max(worst, r)
                assert r <= 1.0, ((B, K), prev_K, use_prev, use_base, r)
                copied = (labels >= prev_K) if use_prev else torch.ones(B, dtype=torch.bool)
                want = base if use_base else F.one_hot(labels, K).float()
                assert torch.equal(tgt.cpu()[copied], want[copied])                      # one-hot / base rows: exact
                assert (~copied).sum() == (labels < prev_K).sum() * use_prev
    print(f'icarl_targets {(B, K)}: err/bar {worst:.3f}')
    record_property('icarl_targets err/bar', worst)


@pytest.mark.parametrize('alpha', [4.0, 0.5])
@pytest.mark.parametrize('bi', range(len(S.LOSS_BK)))
def test_acm_targets_edges(bi, alpha, dev, record_property):
    K_ = _k()
    B, K = S.LOSS_BK[bi]
    g = torch.Generator().manual_seed(24000 + bi)
    labels0 = torch.randint(0, K, (B,), generator=g)
    bg0 = torch.randint(0, K, (B,), generator=g)
    fg0 = torch.rand(B, generator=g)
    worst = 0.0
    for pi, plant in enumerate(('bg = -1', 'bg = label', 'fg = 0', 'fg = 1', 'fg = 0, bg = -1')):
        labels, bg, fg = labels0.clone(), bg0.clone(), fg0.clone()
        row = pi % B
        if 'bg = -1' in plant:
            bg[row] = -1
        if plant == 'bg = label':
            bg[row] = labels[row]
        if 'fg = 0' in plant:
            fg[row] = 0.0
        if plant == 'fg = 1':
            fg[row] = 1.0
        ref = S.acm_targets(labels, bg, fg.double(), alpha, K)
        b = S.bar(ref, S.acm_targets(labels, bg, fg, alpha, K), S.FLOOR_FN, S.CAP_TGT)
        _poison(dev, ((B, K), torch.float32))
        tgt = K_.acm_targets(labels.to(dev), bg.to(dev), fg.to(dev), alpha, K)
        assert tgt.shape == (B, K)
        r = _ratio(tgt, ref, b)
        worst = max(worst, r)
        assert r <= 1.0, ((B, K), alpha, plant, r)
        got = tgt.cpu()[row]
        if 'fg = 0' in plant:                                 # lam = 0: the background's one-hot row (class 0 for -1), exactly
            assert torch.equal(got, F.one_hot(bg[row].clamp(min=0), K).float())
        if plant == 'fg = 1':                                 # lam = 1: the label's one-hot row, exactly
            assert torch.equal(got, F.one_hot(labels[row], K).float())
        if plant == 'bg = -1':
            assert got[0] > 0 or labels[row] == 0
    print(f'acm_targets {(B, K)} alpha={alpha}: err/bar {worst:.3f}')
    record_property('acm_targets err/bar', worst)


# ---- feature-KD MSE ------------------------------------------------------------------------------------------------------

def _kd_grad_bar(gref, bf16):
    b = S.KD_BWD_REL * gref.abs()
    return (b + S.bf16_half_ulp(gref) if bf16 else b).clamp(min=1e-300)


def _kd_check(what, ad, bd_, a64, b64, bf16, dev):
    K_ = _k()
    ref = S.kd_mse(a64, b64)
    _poison(dev, ((1,), torch.float32))
    mse = K_.kd_mse_fwd(ad, bd_)
    assert mse.shape == () and mse.dtype == torch.float32
    r_fwd = _ratio(mse, ref, S.KD_FWD_REL * ref.abs().item())
    print(f'kd_mse {what}: forward err/bar {r_fwd:.3f}')
    assert r_fwd <= 1.0, (what, r_fwd)
    r_bwd = 0.0
    for gdev in (None, 0.375):
        for ghost in (1.0, 3.0):
            gref = S.kd_mse_grad(a64, b64, 1.0 if gdev is None else gdev, ghost)
            gbar = _kd_grad_bar(gref, bf16)
            _poison(dev, (tuple(ad.shape), ad.dtype))
            d = K_.kd_mse_bwd(ad, bd_, None if gdev is None else torch.tensor([gdev], device=dev), ghost)
            assert d.shape == ad.shape and d.stride() == ad.stride() and d.dtype == ad.dtype
            r = _ratio(d, gref, gbar)
            print(f'kd_mse {what} gscale_dev={gdev} gscale_host={ghost}: backward err/bar {r:.3f}')
            assert r <= 1.0, (what, gdev, ghost, r)
            r_bwd = max(r_bwd, r)
    return r_fwd, r_bwd


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('numel', S.KD_NUMELS)
def test_kd_mse_edges(numel, bf16, dev, record_property):
    a, b = S.kd_input(numel, bf16)
    r_fwd, r_bwd = _kd_check(f'{numel} bf16={bf16}', a.to(dev), b.to(dev), a.double(), b.double(), bf16, dev)
    record_property('kd_mse forward err/bar', r_fwd)
    record_property('kd_mse backward err/bar', r_bwd)


@pytest.mark.parametrize('bf16', [False, True])
def test_kd_mse_permuted_pair_and_autograd(bf16, dev, record_property):
    """NCHW views over NHWC storage (what the feature taps hand over), and KDMSEFn with an upstream gradient of 0.25."""
    from bdvcil_amd import functional as Fn
    a, b = S.kd_input(1020, bf16)
    a, b = a.view(3, 5, 17, 4), b.view(3, 5, 17, 4)                          # NHWC
    ad, bd_ = a.to(dev).permute(0, 3, 1, 2), b.to(dev).permute(0, 3, 1, 2)
    assert not ad.is_contiguous()
    a64, b64 = a.double().permute(0, 3, 1, 2), b.double().permute(0, 3, 1, 2)
    r_fwd, r_bwd = _kd_check(f'permuted bf16={bf16}', ad, bd_, a64, b64, bf16, dev)
    record_property('kd_mse forward err/bar', r_fwd)
    record_property('kd_mse backward err/bar', r_bwd)
    cur = ad.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    assert cur.stride() == ad.stride()
    loss = Fn.kd_mse(cur, bd_)
    loss.backward(torch.tensor(0.25, device=dev))
    gref = S.kd_mse_grad(a64, b64, 0.25, 1.0)
    r = _ratio(cur.grad, gref, _kd_grad_bar(gref, bf16))
    record_property('KDMSEFn backward err/bar', r)
    assert r <= 1.0


def test_kd_mse_refuses_a_size_that_is_no_multiple_of_four(dev):
    import bdvcil_amd as bd
    K_ = _k()
    a, b = torch.zeros(6, device=dev), torch.zeros(6, device=dev)
    with pytest.raises(bd._lib.HipExtensionError, match='bdv_kd_mse_fwd: bad argument'):
        K_.kd_mse_fwd(a, b)
    with pytest.raises(bd._lib.HipExtensionError, match='bdv_kd_mse_bwd: bad argument'):
        K_.kd_mse_bwd(a, b, None, 1.0)
    with pytest.raises(ValueError):
        K_.kd_mse_fwd(a, torch.zeros(6, device=dev, dtype=torch.bfloat16))
