"""CPU tests of oracle/step_tail_oracle.py, the reference that tests/test_head_edges_gpu.py, test_loss_edges_gpu.py and
test_optim_edges_gpu.py hold the step's tail against: its fp64 and fp32 runs agree with the goldens made from the reference's own
files, its SGD step and clip rule agree with torch.optim.SGD + clip_grad_norm_ in fp64, every case of the GPU tables meets its margin
condition (so the reference alone keeps the number of dropped cases at zero) and every bar built from the two runs is finite and
positive."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import step_tail_oracle as S
from oracle import tsm_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _close(a, b, tol, atol):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= tol * b.abs().max().item() + atol, (err, b.abs().max().item())


def _runs(fn, tensors, *args):
    """The fp64 and the fp32 run of an oracle function on the same fp32 inputs."""
    return [fn(*[None if t is None else t.to(dt) if t.is_floating_point() else t for t in tensors], *args)
            for dt in (torch.float64, torch.float32)]


def test_heads_and_lsc_loss_agree_with_the_reference_golden():
    gz = np.load(os.path.join(GOLD, 'head_loss_golden.npz'))
    assert int(gz['n_lsc']) >= 1 and int(gz['n_inc']) >= 1
    for i in range(int(gz['n_lsc'])):
        p = f'lsc{i}_'
        x, w, y, eta = (_t(gz[p + k]) for k in ('x', 'w', 'y', 'eta'))
        P, K = int(gz[p + 'P']), w.shape[0]
        for dt in (torch.float64, torch.float32):
            loss = S.lsc_loss(_t(gz[p + 'sim']).to(dt), y, eta.to(dt), 0.6, True)
            head = S.lsc_head(x.to(dt), w.to(dt), K, P, loss['dsim'])
            assert head['sim'].dtype == dt and loss['dsim'].dtype == dt and head['dw'].dtype == dt
            _close(head['sim'], gz[p + 'sim'], 1e-6, 1e-7)
            _close(head['sim'], O.lsc_forward(x.double(), w.double(), K, P), 1e-6, 1e-7)
            _close(loss['loss'], gz[p + 'loss'], 1e-6, 1e-7)
            _close(loss['dsim'], gz[p + 'dsim'], 1e-4, 1e-7)
            _close(loss['deta'], gz[p + 'deta'], 1e-4, 1e-7)
            _close(head['dx'], gz[p + 'dx'], 1e-4, 1e-7)
            _close(head['dw'], gz[p + 'dw'], 1e-4, 1e-7)
            assert head['xnorm'].shape == (x.shape[0],) and head['wnorm'].shape == (K * P,) and head['cosbuf'].shape == (x.shape[0], K * P)
            _close(head['xnorm'], x.double().norm(dim=1), 1e-6, 0)
    for dt in (torch.float64, torch.float32):
        r = S.lsc_loss(_t(gz['hinge_sim']).to(dt), _t(gz['hinge_y']), torch.tensor([10.0], dtype=dt), 0.6, True)
        _close(r['loss'], gz['hinge_loss'], 1e-6, 1e-7)
        _close(r['dsim'], gz['hinge_dsim'], 1e-4, 1e-7)
        _close(r['deta'], gz['hinge_deta'], 1e-4, 1e-7)
    for i in range(int(gz['n_inc'])):
        p = f'inc{i}_'
        x, w, b, dy = (_t(gz[p + k]) for k in ('x', 'w', 'b', 'dy'))
        for r in _runs(S.linear_head, (x, w, b, dy)):
            for k in ('out', 'dx', 'dw', 'db'):
                _close(r[k], gz[p + k], 1e-6, 1e-7)
        nb = S.linear_head(x.double(), w.double(), None, dy.double())
        assert 'db' not in nb and torch.equal(nb['dw'], S.linear_head(x.double(), w.double(), b.double(), dy.double())['dw'])


def test_weighted_lsc_loss_agrees_with_the_reference_golden():
    gz = np.load(os.path.join(GOLD, 'lsc_weights_golden.npz'))
    seen = set()
    for i in range(int(gz['n'])):
        p = f'c{i}_'
        nca, hinge = (bool(v) for v in gz[p + 'cfg'])
        if not nca:                       # the weighted cross-entropy branch is not LSCLoss's kernel
            continue
        cw = _t(gz[p + 'cw'])
        seen.add((hinge, bool((cw < 0).any())))
        eta = torch.tensor([float(gz[p + 'eta'])])
        for r in _runs(S.lsc_loss, (_t(gz[p + 'sim']), _t(gz[p + 'y']), eta), 0.6, hinge, cw):
            _close(r['loss'], gz[p + 'loss'], 1e-6, 1e-7)
            _close(r['dsim'], gz[p + 'dsim'], 1e-4, 1e-7)
            _close(r['deta'], gz[p + 'deta'], 1e-4, 1e-7)
    assert (True, True) in seen           # a negative weight behind the hinge is among them


def test_acm_soft_ce_agrees_with_the_reference_golden():
    gz = np.load(os.path.join(GOLD, 'acm_golden.npz'))
    for i in range(int(gz['n'])):
        p = f'c{i}_'
        score, labels, bg, fg = (_t(gz[p + k]) for k in ('score', 'labels', 'bg', 'fg'))
        for dt in (torch.float64, torch.float32):
            r = S.acm_soft_ce(score.to(dt), labels, bg, fg, float(gz[p + 'alpha']))
            _close(-r['loss'], gz[p + 'loss'], 1e-6, 1e-7)             # the reference's sign: no negation
            _close(-r['dscore'], gz[p + 'dscore'], 1e-4, 1e-7)
            ref = O.acm_smooth_ce(score.to(dt), labels, bg, fg.to(dt), score.shape[1], float(gz[p + 'alpha']))
            _close(r['loss'], -ref, 1e-6, 1e-7)


def test_target_builders_agree_with_tsm_oracle():
    g = torch.Generator().manual_seed(4)
    B, K, prevK = 6, 37, 20
    y = torch.randint(0, K, (B,), generator=g)
    prev = torch.randn(B, K, generator=g)
    bg, fg = torch.randint(-1, K, (B, 1), generator=g), torch.rand(B, 1, generator=g)
    assert torch.allclose(S.icarl_targets(y, K, prev, prevK), O.icarl_targets(y, K, prev, prevK), atol=1e-7)
    base = S.acm_targets(y, bg.view(-1), fg.view(-1), 4.0, K)
    assert torch.allclose(S.icarl_targets(y, K, prev, prevK, base), O.icarl_targets(y, K, prev, prevK, bg, fg), atol=1e-7)
    assert S.icarl_targets(y, K, prev.double(), prevK).dtype == torch.float64
    assert torch.equal(S.icarl_targets(y, K, None, 0), torch.nn.functional.one_hot(y, K).double())


@pytest.mark.parametrize('max_norm', [0.0, 0.5, 1e6])
def test_sgd_oracle_agrees_with_torch_sgd_and_clip_grad_norm(max_norm):
    g = torch.Generator().manual_seed(5)
    shapes = [(7,), (3, 5), (1,), (4, 2, 3)]
    lrs, wds, m, gs = [0.01, 0.05, 0.1, 0.02], [1e-4, 0.0, 1e-4, 5e-4], 0.9, 0.25
    ps = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
    ref_p = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.SGD([dict(params=[p], lr=S.f32(lr), weight_decay=S.f32(wd)) for p, lr, wd in zip(ref_p, lrs, wds)],
                          lr=0.01, momentum=S.f32(m))
    bufs = [torch.zeros_like(p) for p in ps]
    for step in range(3):
        grads = [torch.randn(*s, generator=g).double() * (step + 1) for s in shapes]
        for p, gr in zip(ref_p, grads):
            p.grad = gr * S.f32(gs)
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(ref_p, max_norm).item()
            assert abs(math.sqrt(S.sqnorm(grads)) * S.f32(gs) - total) <= 1e-12 * total
        opt.step()
        coef = S.clip_coef(S.sqnorm(grads), gs, max_norm)
        assert 0 < coef <= 1 and (coef < 1) == (max_norm == 0.5)
        for i in range(len(ps)):
            ps[i], bufs[i], bar_p, bar_b = S.sgd_step(ps[i], grads[i], bufs[i], lrs[i], wds[i], m, gs, coef)
            assert ps[i].dtype == torch.float64 and (bar_p > 0).all() and torch.isfinite(bar_p).all() and torch.isfinite(bar_b).all()
            _close(ps[i], ref_p[i], 1e-12, 0)
            _close(bufs[i], opt.state[ref_p[i]]['momentum_buffer'], 1e-12, 0)
    assert S.clip_coef(4.0, 1.0, 0.0) == 1.0 and S.clip_coef(4.0, 1.0, -1.0) == 1.0 and S.clip_coef(0.0, 1.0, 1.0) == 1.0
    assert S.clip_coef(4.0, 1.0, 3.0) == 1.0 and abs(S.clip_coef(4.0, 0.25, 0.25) - 0.25 / (0.5 + 1e-6)) < 1e-12
    p32 = S.sgd_step(ps[0].float(), grads[0].float(), bufs[0].float(), 0.01, 1e-4, 0.9)[0]
    assert p32.dtype == torch.float32


def test_every_lsc_loss_case_meets_its_margins():
    """What keeps fp32 from flipping an arg-max or the hinge: no case of the GPU table is dropped, each finds a seed among its 20."""
    assert len(S.LSC_LOSS_CASES) == 7 * 3 * 2 * 2 * 3
    later = {}
    for case, (bi, eta, margin, hinge, wkind) in enumerate(S.LSC_LOSS_CASES):
        B, K = S.LOSS_BK[bi]
        (sim, targets, eta_t, cw), t, r64, bars = S.lsc_loss_case(case)
        assert 0 <= t < 20 and sim.abs().max() <= 1 and sim.dtype == torch.float32
        assert S.top2_gap(r64['s']).min().item() >= S.MARGIN
        if K > 1:
            if hinge:
                assert r64['rows'].abs().min().item() >= S.MARGIN
            if wkind == 'negative' and B > 1:
                assert (r64['rows'] >= S.MARGIN).any() and (r64['rows'] < 0).any() and (cw < 0).sum() == 1
        else:
            assert torch.equal(r64['rows'], torch.zeros(B, dtype=torch.float64))
            assert r64['loss'] == 0 and not r64['dsim'].any() and not r64['deta'].any()
        assert (cw is None) == (wkind == 'none') and (cw is None or (cw < 0).any() == (wkind == 'negative'))
        for name, b in bars.items():
            assert math.isfinite(b) and b > 0, (case, name, b)
        if t:
            later[S.LSC_LOSS_CASES[case]] = t
    print('lsc_loss cases that take a later seed:', later)


def test_every_bar_is_finite_and_positive():
    for ci in range(len(S.LSC_CASES)):
        _, r64, bars = S.lsc_case(ci)
        assert set(bars) == {'sim', 'xnorm', 'wnorm', 'cosbuf', 'dx', 'dw'}
        for name, b in bars.items():
            assert r64[name].dtype == torch.float64 and math.isfinite(b) and b > 0, ('lsc', ci, name, b)
            assert b <= (1e-5 if name in ('sim', 'xnorm', 'wnorm', 'cosbuf') else 1e-4) * r64[name].abs().max().item() + 1e-6
    for ci in range(len(S.LINEAR_CASES)):
        for with_bias in (True, False):
            _, r64, bars = S.linear_case(ci, with_bias)
            assert set(bars) == ({'out', 'dx', 'dw', 'db'} if with_bias else {'out', 'dx', 'dw'})
            for name, b in bars.items():
                assert math.isfinite(b) and b > 0, ('linear', ci, with_bias, name, b)
    for bi in range(len(S.LOSS_BK)):
        for kind in S.SOFT_KINDS:
            for scale in S.SCORE_SCALES:
                (score, soft, labels), r64, bars = S.softce_case(bi, kind, scale)
                assert torch.isfinite(r64['loss']) and torch.isfinite(r64['dscore']).all()
                assert (soft is None) == (kind == 'labels') and (labels is None) != (kind == 'labels')
                if kind == 'sum0.7':
                    assert torch.allclose(soft.sum(1), torch.full((score.shape[0],), 0.7), atol=1e-6)
                if scale > 1 and score.numel() > 4:
                    assert score.abs().max() > 60             # exp of it overflows fp32 unless the maximum is subtracted
                for name, b in bars.items():
                    assert math.isfinite(b) and b > 0, ('softce', bi, kind, scale, name, b)
    g = torch.Generator().manual_seed(6)
    for n in S.SGD_NUMELS:
        s64, b = S.sqnorm_bar([torch.randn(n, generator=g)])
        assert math.isfinite(b) and 0 < b <= 1e-5 * s64
    assert S.KD_NUMELS[-1] == 4 * (2 * 262144 + 3) and all(n % 4 == 0 for n in S.KD_NUMELS)


def test_bar_takes_the_tightest_cap_and_the_fp32_deviation():
    ref = torch.tensor([1.0, -2.0], dtype=torch.float64)
    assert S.bar(ref, ref.float(), 2e-7) == 2e-7 * 2
    off = torch.tensor([1.0, -2.0 + 2.0 ** -22])
    assert S.bar(ref, off, 2e-7) == 2e-7 * 2 + 4 * 2.0 ** -22
    assert S.bar(ref, off, 2e-7, (1e-7, 1e-8), (1e-4, 1e-7)) == 1e-7 * 2 + 1e-8
    assert S.bar(torch.zeros(3, dtype=torch.float64), torch.zeros(3), 2e-6, S.CAP_GRAD) == 1e-7
    assert S.f32(0.6) == float(np.float32(0.6)) != 0.6


def test_dyadic_consensus_is_exact_in_fp32():
    g = torch.Generator().manual_seed(7)
    for B, T, K in S.CONSENSUS_CASES:
        if T & (T - 1):
            continue
        s = S.dyadic((B * T, K), g)
        assert torch.equal(S.consensus(s, B, T).double(), S.consensus(s.double(), B, T))
        d = torch.randn(B, K, generator=g)
        assert torch.equal(S.consensus_grad(d, T).double(), S.consensus_grad(d.double(), T))
