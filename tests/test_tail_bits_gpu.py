"""The step-tail kernels' output BITS at small shapes -- heads, losses, the three distillation losses, the optimizer and the
representation path -- against hashes recorded before their shared pieces were given one definition each (csrc/reduce_pieces.h;
tests/golden/tail_bits.json -- ``python tests/test_tail_bits_gpu.py`` on a GPU re-records it from the library ``BDVCIL_LIB_PATH``
names).  The other tail suites allow tolerances against fp64; this one holds the outputs to what the library computed before, bit for
bit: the association order of every block sum and the contraction setting of every file are part of a kernel's result.  Every call goes
through the Python bindings (FusedSGD for the optimizer); inputs are seeded on the CPU.  Each shape is the smallest at which its path
can go wrong:

  lsc_fwd / lsc_bwd           N 5, D 70, K 3, P 2 (a partial row block of HEAD_RB = 4, D past one lane stride and no multiple of 64);
                              N 1, D 1, K 1, P 1
  linear_fwd / linear_bwd     N 5, D 70, K 9 (a second class block of 8), with bias, beta_w 0 and 0.5
  lsc_loss                    B 6, K 70 (a wave takes two rows), hinge off / on, without / with class_weights (some negative, so
                              the hinge cuts), row 0 with two equal maxima
  softce_loss                 B 6, K 70, soft targets; labels
  icarl_targets               B 6, K 70, prev_K 3: old and new labels in both blocks; without / with base_targets
  acm_targets                 B 6, K 70, one background label of -1
  softmax_mean                B 5, n 3, K 70, softmax on / off
  topk_acc                    B 6, K 70
  kd_mse_fwd / kd_mse_bwd     numel 4; 4 * (2 * 256 + 3) in fp32 and bf16; 4 * (1024 * 256 + 5): the grid is capped, the stride loop
                              runs twice
  kd_tc_fwd / kd_tc_bwd       (N 4, T 2, C 8, 3x3) channels-last in fp32 and bf16; the (N, D) form, N 4, T 2, D 12; a plainly
                              contiguous cur (the copy path)
  tc_sqgrad_accum             C 8 (16-wide slab) and C 256 (64-wide slab), N 4, T 2, 3x3, a non-zero S
  pod_spatial_fwd / _bwd      N 3, C 8 / 68 (a second, partial slab), H 5, W 3 / 9 / 17 / 33 (the four JW instantiations), fp32 / bf16
                              (the staged loads); one pair with cur == prev
  pod_flat                    N 5, D 260; the (N, D, 1, 1) form
  FusedSGD                    tensors of 1, 255 and 8193 (one past CHUNKS * 256) elements, two clipped steps: parameters, momentum
                              buffers, squared norm, clip coefficient
  repr_from_features          B 2, crops 3, T 2, D 260
  nme_classify                K 5, two equal class means (the tie)
  class_means                 one empty class
  herding_select              n 6, D 70, m 4, cosine / Euclidean"""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tail_bits.json')

CASES = ([('lsc', '5x70x3x2'), ('lsc', '1x1x1x1'), ('linear', 0.0), ('linear', 0.5)]
         + [('lsc_loss', h, w) for h in ('nohinge', 'hinge') for w in ('noweights', 'weights')]
         + [('softce', 'soft'), ('softce', 'labels'), ('icarl', 'onehot'), ('icarl', 'base'), ('acm',), ('softmax_mean', 'softmax'),
            ('softmax_mean', 'mean'), ('topk',), ('kd_mse', 'f32', 4), ('kd_mse', 'f32', 4 * (2 * 256 + 3)), ('kd_mse', 'bf16', 4 * (2 * 256 + 3)),
            ('kd_mse', 'f32', 4 * (1024 * 256 + 5)), ('kd_tc', 'f32'), ('kd_tc', 'bf16'), ('kd_tc', 'nd'), ('kd_tc', 'copy'),
            ('tc_sqgrad', 8), ('tc_sqgrad', 256)]
         + [('pod_spatial', dt, C, W) for dt in ('f32', 'bf16') for C in (8, 68) for W in (3, 9, 17, 33)]
         + [('pod_spatial', 'same'), ('pod_flat', 'nd'), ('pod_flat', 'nd11'), ('sgd',), ('repr',), ('nme',), ('class_means',),
            ('herding', 'cosine'), ('herding', 'euclidean')])


def _key(case):
    return '/'.join(map(str, case))


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def _shas(**tensors):
    return {n: _sha(t) for n, t in tensors.items()}


def tail_hashes(case, dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd.optim import FusedSGD
    gen = torch.Generator().manual_seed(7000 + CASES.index(case))
    rn = lambda *s: torch.randn(*s, generator=gen)                                          # noqa: E731
    ri = lambda hi, *s: torch.randint(0, hi, s, dtype=torch.int64, generator=gen)           # noqa: E731
    one = lambda v: torch.tensor([v], dtype=torch.float32).to(dev)                          # noqa: E731
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)                  # noqa: E731
    kind = case[0]
    if kind == 'lsc':
        N, D, Kc, P = map(int, case[1].split('x'))
        x, w, dsim = rn(N, D).to(dev), rn(Kc, P * D).to(dev), rn(N, Kc).to(dev)
        sim, xnorm, wnorm, cosbuf = K.lsc_fwd(x, w, Kc, P)
        dx, dw = K.lsc_bwd(dsim, x, w, xnorm, wnorm, cosbuf, Kc, P)
        out = _shas(sim=sim, xnorm=xnorm, wnorm=wnorm, cosbuf=cosbuf, dx=dx, dw=dw)
    elif kind == 'linear':
        N, D, Kc, beta = 5, 70, 9, case[1]
        x, w, b, dout = rn(N, D).to(dev), rn(Kc, D).to(dev), rn(Kc).to(dev), rn(N, Kc).to(dev)
        y = K.linear_fwd(x, w, b)
        dw0, db0 = (rn(Kc, D).to(dev), rn(Kc).to(dev)) if beta else (None, None)
        dx, dw, db = K.linear_bwd(dout, x, w, dw=dw0, db=db0, beta_w=beta)
        out = _shas(out=y, dx=dx, dw=dw, db=db)
    elif kind == 'lsc_loss':
        B, Kc = 6, 70
        sim = rn(B, Kc)
        sim[0, 3] = sim[0, 40] = 9.0                                                        # two equal maxima: the first index wins
        weights = rn(Kc).to(dev) if case[2] == 'weights' else None
        loss, dsim, deta = K.lsc_loss(sim.to(dev), ri(Kc, B).to(dev), one(1.7), 0.25, case[1] == 'hinge', weights)
        out = _shas(loss=loss, dsim=dsim, deta=deta)
    elif kind == 'softce':
        B, Kc = 6, 70
        score = rn(B, Kc).to(dev)
        if case[1] == 'soft':
            loss, dscore = K.softce_loss(score, soft_targets=torch.softmax(rn(B, Kc), 1).to(dev))
        else:
            loss, dscore = K.softce_loss(score, labels=ri(Kc, B).to(dev))
        out = _shas(loss=loss, dscore=dscore)
    elif kind == 'icarl':
        B, Kc = 6, 70
        labels = torch.tensor([0, 5, 2, 69, 1, 30])
        base = torch.softmax(rn(B, Kc), 1).to(dev) if case[1] == 'base' else None
        out = _shas(targets=K.icarl_targets(labels.to(dev), rn(B, Kc).to(dev), 3, Kc, base_targets=base))
    elif kind == 'acm':
        B, Kc = 6, 70
        bg = ri(Kc, B)
        bg[2] = -1
        out = _shas(targets=K.acm_targets(ri(Kc, B).to(dev), bg.to(dev), torch.rand(B, generator=gen).to(dev), 0.8, Kc))
    elif kind == 'softmax_mean':
        out = _shas(out=K.softmax_mean(rn(5 * 3, 70).to(dev), 5, 3, apply_softmax=case[1] == 'softmax'))
    elif kind == 'topk':
        out = _shas(acc=K.topk_acc(rn(6, 70).to(dev), ri(70, 6).to(dev)))
    elif kind == 'kd_mse':
        dt = torch.bfloat16 if case[1] == 'bf16' else torch.float32
        cur, prev = rn(case[2]).to(dt).to(dev), rn(case[2]).to(dt).to(dev)
        out = _shas(mse=K.kd_mse_fwd(cur, prev), dcur=K.kd_mse_bwd(cur, prev, one(0.6), 0.7))
    elif kind == 'kd_tc':
        N, T, C = 4, 2, 8
        if case[1] == 'nd':
            C = 12
            cur, prev = rn(N, C).to(dev), rn(N, C).to(dev)
        elif case[1] == 'copy':
            cur, prev = rn(N, C, 3, 3).to(dev), rn(N, C, 3, 3).to(dev)
        else:
            dt = torch.bfloat16 if case[1] == 'bf16' else torch.float32
            cur, prev = cl(rn(N, C, 3, 3).to(dt)), cl(rn(N, C, 3, 3).to(dt))
        A = (torch.rand(T, C, generator=gen) + 0.5).to(dev)
        d = K.kd_tc_bwd(cur, prev, A, one(0.6))
        out = dict(_shas(loss=K.kd_tc_fwd(cur, prev, A), dcur=d), same_strides=d.stride() == cur.stride())
    elif kind == 'tc_sqgrad':
        N, T, C = 4, 2, case[1]
        S = torch.rand(T, C, generator=gen).to(dev)
        out = _shas(S=K.tc_sqgrad_accum(S, cl(rn(N, C, 3, 3)), 0.5))
    elif kind == 'pod_spatial':
        if case[1] == 'same':
            cur = cl(rn(3, 8, 5, 9))
            prev = cur.clone(memory_format=torch.preserve_format)
        else:
            dt = torch.bfloat16 if case[1] == 'bf16' else torch.float32
            cur, prev = cl(rn(3, case[2], 5, case[3]).to(dt)), cl(rn(3, case[2], 5, case[3]).to(dt))
        loss, G, a = K.pod_spatial_fwd(cur, prev)
        d = K.pod_spatial_bwd(cur, G, one(0.6))
        out = dict(_shas(loss=loss, G=G, dcur=d), same_strides=d.stride() == cur.stride())
    elif kind == 'pod_flat':
        shape = (5, 260) if case[1] == 'nd' else (5, 260, 1, 1)
        loss, d = K.pod_flat(rn(*shape).to(dev), rn(*shape).to(dev))
        out = _shas(loss=loss, dcur_unit=d)
    elif kind == 'sgd':
        params = [torch.nn.Parameter(rn(n).to(dev)) for n in (1, 255, 8193)]
        opt = FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
        out = {}
        for step in (0, 1):
            for p in params:
                p.grad = rn(p.numel()).to(dev)
            opt.clip_grad_norm_(1.0)
            opt.step()
            out.update(_shas(**{f'sqnorm{step}': opt._sqnorm, f'coef{step}': opt._coef}))
        for n, p in zip((1, 255, 8193), params):
            out.update(_shas(**{f'param{n}': p, f'buf{n}': opt.state[p]['momentum_buffer']}))
    elif kind == 'repr':
        rp, mc = K.repr_from_features(rn(2 * 3 * 2, 260).to(dev), 2, 3, 2)
        out = _shas(repr=rp, mean_crops=mc)
    elif kind == 'nme':
        means = rn(5, 70)
        means[3] = means[1]
        rp = rn(3, 2, 70)
        rp[0] = means[1] + 0.01 * rn(2, 70)                                                  # sample 0 lies at the doubled mean
        sim, pred = K.nme_classify(rp.to(dev), means.to(dev))
        out = _shas(sim=sim, pred=pred)
    elif kind == 'class_means':
        out = _shas(means=K.class_means(rn(6, 70).to(dev), torch.tensor([0, 3, 1, 0, 3, 3]).to(dev), 4))      # class 2 is empty
    else:
        assert kind == 'herding'
        cm, idx, dist = K.herding_select(rn(6, 70).to(dev), 4, case[1] == 'cosine')
        out = _shas(class_mean=cm, indices=idx, dist=dist)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)['bits']


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(_key(c) for c in CASES) and len({_key(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=_key)
def test_tail_output_bits(case, golden, dev):
    assert tail_hashes(case, dev) == golden[_key(case)]


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    table = {'bits': {_key(c): tail_hashes(c, torch.device('cuda:0')) for c in CASES}}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', len(table['bits']), 'cases')
