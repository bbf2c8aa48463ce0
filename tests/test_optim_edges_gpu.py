"""Edge sweep of csrc/optim.hip -- multi_sqnorm_partial / sqnorm_finalize, clip_coef_kernel, multi_sgd_kernel -- and of FusedSGD
around them, against the fp64 run of oracle/step_tail_oracle.py (held against torch.optim.SGD + clip_grad_norm_ in
tests/test_step_tail_cpu.py) and, for FusedSGD, against fp64 torch.optim.SGD + clip_grad_norm_ on copies.  A tensor is walked in 32
chunks of 256: the sizes sit on both sides of a block, of one pass of 8192 and of three passes; tables hold one tensor, 161 tensors
and slices of one buffer at offsets that are no multiple of 4 elements.

Bars
  * exact: the coefficient 1 (max_norm <= 0, a norm below max_norm, all-zero gradients), tensors a step must not touch;
  * multi_sqnorm: 2e-7 * max(1, scale) + 4 x the deviation of the fp32 CPU sum from the fp64 sum, at most 1e-5 relative; the total
    norm and a coefficient below 1 are sqrt / division of it: half its relative bar plus 4 * 2^-24;
  * SGD, per element, u = 2^-24: 4u (|g gs coef| + |wd p| + |m b|) on the buffer, |lr| times that plus 2u (|p| + |lr b'|) on the
    parameter -- the five roundings of the update, three more for gs * coef and the products.  Every step is checked from the
    kernel's own previous state copied to fp64 (for FusedSGD the reference's parameters and buffers are reset to it after every
    step), so the bars do not compound.  multi_sgd is given the kernel's own coefficient; in a clipped FusedSGD step the
    reference's coefficient is its own, and the buffer's bar grows by |g gs| times the coefficient's bar.

Largest error / bar observed on an MI355X (recorded per test with record_property):
  multi_sqnorm 0.192 (a single element), clip_coef 0.241; multi_sgd parameter 0.498, buffer 0.471; FusedSGD parameter 0.485, buffer
  0.475, total norm 0.105; everything else is exact.
"""
import math

import pytest
import torch

from oracle import step_tail_oracle as S

pytestmark = pytest.mark.gpu

U = S.U


def _k():
    from bdvcil_amd import kernels as K
    return K


def _ratio(got, ref64, bar):
    """Largest |got - ref| / bar (bar: a float or a tensor of ref's shape); shapes and NaN positions must agree."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), 'NaN positions differ'
    err = torch.nan_to_num((got - ref64).abs(), nan=0.0)
    return (err / bar).max().item() if err.numel() else 0.0


def _ptrs(tensors, dev):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=dev)


def _slices(numels, dev, g, offset=0, zero=False):
    """Tensors of the given sizes cut out of ONE device buffer (allocations are 16-byte aligned): back to back for ``offset`` 0, else
    ``offset`` or more elements apart and every one starting off a multiple of 4 elements.  Returns (device views, CPU copies, starts)."""
    starts, at = [], 0
    for n in numels:
        if offset and at % 4 == 0:
            at += 1
        starts.append(at)
        at += n + offset
    flat = torch.zeros(at + 4) if zero else torch.randn(at + 4, generator=g)
    dflat = flat.to(dev)
    return [dflat[s:s + n] for s, n in zip(starts, numels)], [flat[s:s + n].clone() for s, n in zip(starts, numels)], starts


TABLES = {
    'one of each size': (S.SGD_NUMELS, 0),
    '161 small tensors': ([(i * 37) % 300 + 1 for i in range(161)], 0),
    'odd offsets in one buffer': ([5, 255, 257, 8193, 1, 1023, 3 * 8192 + 17], 3),
    'a single element': ([1], 0),
}
for n in S.SGD_NUMELS:
    TABLES[f'alone: {n}'] = ([n], 1)


@pytest.mark.parametrize('table', list(TABLES))
def test_multi_sqnorm_and_clip_coef(table, dev, record_property):
    K_ = _k()
    numels, offset = TABLES[table]
    g = torch.Generator().manual_seed(5000 + len(numels) + numels[0])
    dg, cg, _ = _slices(numels, dev, g, offset)
    if offset:
        assert all(t.data_ptr() % 16 for t in dg)
    n = len(numels)
    nd = torch.tensor(numels, dtype=torch.int64, device=dev)
    sq = torch.full((1,), float('nan'), device=dev)
    K_.multi_sqnorm(_ptrs(dg, dev), nd, n, sq)
    s64, b = S.sqnorm_bar(cg)
    r_sq = _ratio(sq, torch.tensor([s64], dtype=torch.float64), b)
    rel = b / s64
    print(f'multi_sqnorm {table}: sum {s64:.6g}, bar {rel:.2e} relative, err/bar {r_sq:.3f}')
    record_property('multi_sqnorm err/bar', r_sq)
    assert r_sq <= 1.0
    coef = torch.full((1,), float('nan'), device=dev)
    norm = math.sqrt(s64)
    worst = 0.0
    for gs in (1.0, 0.25):
        for max_norm in (0.0, -1.0, 2.0 * norm * gs, 1.0000001 * norm * gs + 1e-5, 0.5 * norm * gs, 1e-3 * norm * gs):
            coef.fill_(float('nan'))
            K_.clip_coef(sq, gs, max_norm, coef)
            want = S.clip_coef(s64, gs, max_norm)
            if max_norm <= 0 or max_norm >= 2.0 * norm * gs:
                assert want == 1.0 and coef.item() == 1.0, (gs, max_norm, coef.item())     # exactly 1: nothing is scaled
            else:
                r = _ratio(coef, torch.tensor([want], dtype=torch.float64), want * (0.5 * rel + 4 * U))
                worst = max(worst, r)
                assert r <= 1.0 and coef.item() <= 1.0, (gs, max_norm, coef.item(), want, r)
    print(f'clip_coef {table}: err/bar {worst:.3f}')
    record_property('clip_coef err/bar', worst)


def test_clip_coef_of_all_zero_gradients(dev):
    K_ = _k()
    numels = [1, 257, 8193]
    dg, _, _ = _slices(numels, dev, None, 1, zero=True)
    sq = torch.full((1,), float('nan'), device=dev)
    K_.multi_sqnorm(_ptrs(dg, dev), torch.tensor(numels, dtype=torch.int64, device=dev), len(numels), sq)
    assert sq.item() == 0.0
    coef = torch.full((1,), float('nan'), device=dev)
    for gs, max_norm in ((1.0, 1.0), (0.25, 1e-3), (1.0, 0.0)):
        K_.clip_coef(sq, gs, max_norm, coef)
        assert coef.item() == 1.0 == S.clip_coef(0.0, gs, max_norm)                        # max_norm / 1e-6 is far above 1


@pytest.mark.parametrize('use_coef', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('table', ['one of each size', '161 small tensors', 'odd offsets in one buffer'])
def test_multi_sgd_steps(table, momentum, wd, use_coef, dev, record_property):
    K_ = _k()
    numels, offset = TABLES[table]
    n = len(numels)
    g = torch.Generator().manual_seed(5100 + n)
    dp, _, starts = _slices(numels, dev, g, offset)
    db, _, _ = _slices(numels, dev, None, offset, zero=True)
    guard = dp[0]._base.clone()                                               # the whole parameter buffer, gaps included
    lrs = [0.01 * (1 + i % 7) for i in range(n)]                              # per-tensor lr; every third tensor without decay
    wds = [0.0 if i % 3 == 2 else wd for i in range(n)]
    lr_t, wd_t = torch.tensor(lrs, device=dev), torch.tensor(wds, device=dev)
    nd = torch.tensor(numels, dtype=torch.int64, device=dev)
    pp, bp = _ptrs(dp, dev), _ptrs(db, dev)
    gs = 0.25 if use_coef else 1.0
    worst_p = worst_b = 0.0
    for step in range(3):
        dg, _, _ = _slices(numels, dev, g, offset)                            # fresh gradients every step
        coef_t, coef = None, 1.0
        if use_coef:
            coef_t = torch.tensor([0.625 / (step + 1)], device=dev)
            coef = float(coef_t.item())
        prev_p = [t.cpu().double() for t in dp]                               # the kernel's own state before the step
        prev_b = [t.cpu().double() for t in db]
        grads = [t.cpu().double() for t in dg]
        K_.multi_sgd(pp, _ptrs(dg, dev), bp, nd, lr_t, wd_t, n, momentum, gs, coef_t)
        torch.cuda.synchronize()
        for i in range(n):
            p2, b2, bar_p, bar_b = S.sgd_step(prev_p[i], grads[i], prev_b[i], lr_t[i].item(), wd_t[i].item(), momentum, gs, coef)
            worst_p = max(worst_p, _ratio(dp[i], p2, bar_p.clamp(min=1e-300)))
            worst_b = max(worst_b, _ratio(db[i], b2, bar_b.clamp(min=1e-300)))
            assert torch.equal(dg[i].cpu().double(), grads[i])                # gradients are read only
    print(f'multi_sgd {table} m={momentum} wd={wd} coef={use_coef}: parameter err/bar {worst_p:.3f}, buffer err/bar {worst_b:.3f}')
    record_property('multi_sgd parameter err/bar', worst_p)
    record_property('multi_sgd buffer err/bar', worst_b)
    assert worst_p <= 1.0 and worst_b <= 1.0
    if offset:                                                                # nothing between or around the tensors was written
        now = dp[0]._base
        mask = torch.ones_like(guard, dtype=torch.bool)
        for at, k in zip(starts, numels):
            mask[at:at + k] = False
        assert torch.equal(now[mask], guard[mask]) and not db[0]._base[mask].any()


# ---- FusedSGD ------------------------------------------------------------------------------------------------------------

def test_fused_sgd_steps_against_fp64_torch_sgd(dev, record_property):
    """Ten steps with freshly allocated gradients: the first six keep one active set, so the four-slot ring of pinned pointer tables
    wraps; a parameter has no gradient on steps 6 and 9 (the active count changes, twice each way); a MultiStepLR milestone after
    step 2; a channels-last gradient for a contiguous 4-D parameter and the reverse on every step (layout mismatch);
    set_grad_scale(0.5) from step 3 on; a clipped step (1) followed by an unclipped one (2), which must not reuse the coefficient;
    steps 1, 3, 4 and 6 clip (4: max_norm above the norm, coefficient exactly 1)."""
    import bdvcil_amd as bd
    g = torch.Generator().manual_seed(5200)
    shapes = [(8, 4, 3, 3), (6, 5, 3, 3), (257, 5), (1,), (8193,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    params = [t.to(dev) for t in init]
    params[1] = params[1].contiguous(memory_format=torch.channels_last)
    params = [torch.nn.Parameter(t) for t in params]
    m, lr0, lr1, wd = 0.9, 0.0625, 0.25, 1e-4                                 # the lrs and gamma = 0.5 are exact in fp32 and fp64
    opt = bd.FusedSGD([dict(params=params[:2], lr=lr0, weight_decay=wd), dict(params=params[2:], lr=lr1, weight_decay=0.0)],
                      lr=lr0, momentum=m)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3], gamma=0.5)
    ref = [torch.nn.Parameter(t.double()) for t in init]
    ropt = torch.optim.SGD([dict(params=ref[:2], lr=lr0, weight_decay=S.f32(wd)), dict(params=ref[2:], lr=lr1, weight_decay=0.0)],
                           lr=lr0, momentum=S.f32(m))
    rsched = torch.optim.lr_scheduler.MultiStepLR(ropt, milestones=[3], gamma=0.5)
    group_of = [0, 0, 1, 1, 1]
    bufs = [torch.zeros_like(t, dtype=torch.float64) for t in init]
    worst = dict(p=0.0, b=0.0, norm=0.0)
    for step in range(10):
        gs = 0.5 if step >= 3 else 1.0
        opt.set_grad_scale(gs)
        active = [i for i in range(5) if not (i == 4 and step in (6, 9))]
        grads = {i: torch.randn(*shapes[i], generator=g) * (3.0 if step == 1 else 1.0) for i in active}
        for i in range(5):
            if i not in grads:
                params[i].grad = ref[i].grad = None
                continue
            gd = grads[i].to(dev)                                              # a fresh allocation every step
            if i == 0:
                gd = gd.contiguous(memory_format=torch.channels_last)          # channels-last gradient, contiguous parameter
            assert (i in (0, 1)) == (gd.stride() != params[i].stride())        # ... and a contiguous one for the channels-last parameter
            params[i].grad = gd
            ref[i].grad = grads[i].double() * gs
        prev_p = [p.detach().cpu().double() for p in params]
        max_norm = {1: 1.0, 3: 0.75, 4: 1e4, 6: 0.5}.get(step)
        coef, coef_bar = 1.0, 0.0
        if max_norm is not None:
            total = opt.clip_grad_norm_(max_norm)
            rtotal = torch.nn.utils.clip_grad_norm_([ref[i] for i in active], max_norm).double()
            s64, b = S.sqnorm_bar([grads[i] for i in active])
            rel = 0.5 * b / s64 + 4 * U
            coef = S.clip_coef(s64, gs, max_norm)
            assert abs(rtotal.item() - math.sqrt(s64) * gs) <= 1e-12 * rtotal.item()
            assert (coef < 1.0) == (step != 4)
            r = _ratio(total.reshape(()), rtotal.reshape(()), rel * rtotal.item())
            worst['norm'] = max(worst['norm'], r)
            assert r <= 1.0, (step, r)
            got_coef = opt._coef.item()
            if coef < 1.0:
                coef_bar = coef * rel
                assert abs(got_coef - coef) <= coef_bar, (step, got_coef, coef)
            else:
                assert got_coef == 1.0
        opt.step()
        ropt.step()
        torch.cuda.synchronize()
        lrs = [grp['lr'] for grp in ropt.param_groups]
        assert lrs == [grp['lr'] for grp in opt.param_groups] == ([lr0, lr1] if step < 3 else [lr0 / 2, lr1 / 2])
        for i in range(5):
            p_now = params[i].detach()
            if i not in grads:                                                 # no gradient: neither the parameter nor its buffer moves
                assert torch.equal(p_now.cpu().double(), prev_p[i]) and torch.equal(ref[i].detach(), prev_p[i])
            else:
                gi = group_of[i]
                _, _, bar_p, bar_b = S.sgd_step(prev_p[i], grads[i].double(), bufs[i], lrs[gi], (wd, 0.0)[gi], m, gs, coef)
                bar_b = bar_b + (grads[i].double() * gs).abs() * coef_bar
                bar_p = bar_p + lrs[gi] * (grads[i].double() * gs).abs() * coef_bar
                rb = ropt.state[ref[i]]['momentum_buffer']
                worst['p'] = max(worst['p'], _ratio(p_now, ref[i].detach(), bar_p.clamp(min=1e-300)))
                worst['b'] = max(worst['b'], _ratio(opt.state[params[i]]['momentum_buffer'], rb, bar_b.clamp(min=1e-300)))
                assert params[i].grad.stride() == params[i].stride()           # the mismatching gradient was replaced, not the parameter
                bufs[i] = opt.state[params[i]]['momentum_buffer'].detach().cpu().double()
                rb.copy_(bufs[i])                                              # the next step starts from the kernel's own state
            ref[i].data.copy_(p_now.cpu().double())
        print(f'FusedSGD step {step}: active {len(active)}, coef {coef:.6f}, worst so far {worst}')
        assert worst['p'] <= 1.0 and worst['b'] <= 1.0, (step, worst)
        sched.step()
        rsched.step()
    assert params[1].is_contiguous(memory_format=torch.channels_last) and params[0].is_contiguous()
    for k, v in worst.items():
        record_property(f'FusedSGD {k} err/bar', v)
