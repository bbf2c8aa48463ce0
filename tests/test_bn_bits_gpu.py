"""The BatchNorm kernels' output BITS at small shapes, against hashes recorded before csrc/bn.hip was folded onto shared helpers and
table-driven launches (tests/golden/bn_bits.json; ``python tests/test_bn_bits_gpu.py`` on a GPU re-records them).  An expression that
is re-associated, a reduction that sums in another order or a launch that reaches another instantiation with other arithmetic changes
a hash; parity with the CPU oracle is the business of the other BatchNorm suites.  Every call goes through ``kernels.py``; inputs are
seeded on the CPU.  Each shape is the smallest at which its code path can still go wrong:

  bn_train_stats       (1, 64), (300, 128), (257, 512): 16 / 32 / 64 column vectors per block, one and two column chunks, a ragged
                       last row block; the running statistics are hashed too
  bn_train_finalize    1 / 1025 / 2049 partial rows (1025 enters the four-chain loop and its tail) x C 64 / 256 x 1 / 2 / 16 blocks
                       per channel group, with and without running statistics
  bn_apply             every (relu, residual, mask, res_affine) form x fp32 / bf16 x BDVCIL_BN_NT unset / 0 / 1
  bn_backward          no ReLU / mask / sign derived from y x own statistics / 3 given tile rows x 1 / 4 finalize blocks x fp32 / bf16,
                       once with BDVCIL_BN_NT=0, once accumulating into given dgamma / dbeta
  bn_backward_pair     C = 64 (four units per thread, ragged against the 4 L span) and C = 768 (256 % (C / 4) != 0: the plain kernel)
  bn_eval_backward     sign {none, mask, activation} x want_dz x want_params in fp32, two of them in bf16, two with BDVCIL_BN_NT=0
  bn_backward_maxpool  (1, 9, 9, 64): odd size, edge pixels without a right / lower neighbour; (2, 8, 10, 128)
  relu_bwd, add        with and without ``add``, fp32 and bf16

BDVCIL_BN_NT is read by the library per call; it is set for the one call and restored."""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bn_bits.json')
UNSET = None
DTYPES = ('f32', 'bf16')
APPLY_FORMS = ('relu_mask', 'relu_res_mask', 'relu_res_affine', 'res', 'plain')
SIGNS = ('none', 'mask', 'act')


def _cases():
    c = [('train_stats', M, C) for M, C in ((1, 64), (300, 128), (257, 512))]
    c += [('train_finalize', rows, C, S, run) for rows in (1, 1025, 2049) for C in (64, 256) for S in (1, 2, 16) for run in (0, 1)]
    c += [('apply', C, form, dt, nt) for C in (64, 256) for form in APPLY_FORMS for dt in DTYPES for nt in (UNSET, '0', '1')]
    c += [('backward', M, C, relu, part, S, dt, UNSET, 0) for M, C in ((37, 64), (300, 256)) for relu in ('none', 'mask', 'affine')
          for part in (0, 1) for S in (1, 4) for dt in DTYPES]
    c += [('backward', 37, 64, 'mask', 0, 1, 'f32', '0', 0), ('backward', 37, 64, 'mask', 0, 1, 'f32', UNSET, 1)]
    c += [('pair', C, dt, part) for C in (64, 768) for dt in DTYPES for part in (0, 1)]
    c += [('eval_backward', sign, dz, params, 'f32', UNSET) for sign in SIGNS for dz in (0, 1) for params in (0, 1)]
    c += [('eval_backward', 'mask', 1, 1, 'bf16', UNSET), ('eval_backward', 'act', 0, 0, 'bf16', UNSET),
          ('eval_backward', 'mask', 1, 0, 'f32', '0'), ('eval_backward', 'act', 1, 1, 'f32', '0')]
    c += [('maxpool', shape, dt, S) for shape in ((1, 9, 9, 64), (2, 8, 10, 128)) for dt in DTYPES for S in (1, 2)]
    c += [('relu_bwd', add, dt) for add in (0, 1) for dt in DTYPES] + [('add', dt) for dt in DTYPES]
    return c


CASES = _cases()


def _key(case):
    return '/'.join('x'.join(map(str, v)) if isinstance(v, tuple) else 'unset' if v is None else str(v) for v in case)


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def _bits(n, gen):
    """n sign bits as n / 32 int32 words (the layout of ``bn_apply(want_mask=True)``)."""
    return torch.from_numpy(np.packbits((torch.randn(n, generator=gen) > 0).numpy(), bitorder='little').view(np.int32).copy())


@contextlib.contextmanager
def _bn_nt(value):
    saved = os.environ.pop('BDVCIL_BN_NT', None)
    if value is not None:
        os.environ['BDVCIL_BN_NT'] = value
    try:
        yield
    finally:
        os.environ.pop('BDVCIL_BN_NT', None)
        if saved is not None:
            os.environ['BDVCIL_BN_NT'] = saved


def _act(t, dt):
    return t.to(torch.bfloat16) if dt == 'bf16' else t


def _stats(C, gen):
    """(gamma, mean, invstd) of C channels."""
    return torch.randn(C, generator=gen), torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5


def bn_hashes(case, dev):
    from bdvcil_amd import kernels as K
    gen = torch.Generator().manual_seed(7000 + CASES.index(case))
    kind = case[0]
    d = lambda t: t.to(dev) if t is not None else None                                      # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=gen)                                          # noqa: E731
    out = {}
    if kind == 'train_stats':
        _, M, C = case
        rm, rv = d(rn(C)), d(torch.rand(C, generator=gen) + 0.5)
        r = K.bn_train_stats(d(rn(M, C)), d(rn(C)), d(rn(C)), 1e-5, 0.1, rm, rv)
        out = dict(zip(('mean', 'invstd', 'scale', 'shift'), map(_sha, r)), running_mean=_sha(rm), running_var=_sha(rv))
    elif kind == 'train_finalize':
        _, rows, C, S, run = case
        partial = torch.stack((rn(rows, C), rn(rows, C).square() + 1.0))
        rm, rv = (d(rn(C)), d(torch.rand(C, generator=gen) + 0.5)) if run else (None, None)
        r = K.bn_train_finalize(d(partial), rows * 4, d(rn(C)), d(rn(C)), 1e-5, 0.1, rm, rv, splits=S)
        out = dict(zip(('mean', 'invstd', 'scale', 'shift'), map(_sha, r)))
        if run:
            out.update(running_mean=_sha(rm), running_var=_sha(rv))
    elif kind == 'apply':
        _, C, form, dt, nt = case
        y, res = _act(rn(37, C), dt), _act(rn(37, C), dt)
        scale, shift, rs, rb = rn(C), rn(C), rn(C), rn(C)
        relu, has_res, mask = form.startswith('relu'), 'res' in form, form.endswith('mask')
        with _bn_nt(nt):
            r = K.bn_apply(d(y), d(scale), d(shift), res=d(res) if has_res else None, relu=relu, want_mask=mask,
                           res_affine=(d(rs), d(rb)) if form == 'relu_res_affine' else None)
            torch.cuda.synchronize()
        out = dict(out=_sha(r[0]), mask=_sha(r[1])) if mask else dict(out=_sha(r))
    elif kind == 'backward':
        _, M, C, relu, part, S, dt, nt, acc = case
        dout, y = _act(rn(M, C), dt), _act(rn(M, C), dt)
        gamma, mean, invstd = _stats(C, gen)
        mask = _bits(M * C, gen) if relu == 'mask' else None
        affine = (d(rn(C)), d(rn(C))) if relu == 'affine' else None
        stat = d(torch.stack((rn(3, C), rn(3, C)))) if part else None
        dg, db = (d(rn(C)), d(rn(C))) if acc else (None, None)
        with _bn_nt(nt):
            r = K.bn_backward(d(dout), d(mask), d(y), d(gamma), d(mean), d(invstd), relu != 'none', dgamma=dg, dbeta=db,
                              beta_acc=0.5 if acc else 0.0, stat_partial=stat, relu_affine=affine, splits=S)
            torch.cuda.synchronize()
        out = dict(zip(('dy', 'dgamma', 'dbeta'), map(_sha, r)))
    elif kind == 'pair':
        _, C, dt, part = case
        M = 37
        dout, ya, yb = (_act(rn(M, C), dt) for _ in range(3))
        sa, sb = _stats(C, gen), _stats(C, gen)
        stat = d(torch.stack((rn(3, C), rn(3, C)))) if part else None
        ra, rb = K.bn_backward_pair(d(dout), d(_bits(M * C, gen)), d(ya), *map(d, sa), d(yb), *map(d, sb), stat_partial_a=stat)
        out = dict(zip(('dya', 'dgamma_a', 'dbeta_a', 'dyb', 'dgamma_b', 'dbeta_b'), map(_sha, ra + rb)))
    elif kind == 'eval_backward':
        _, sign, dz, params, dt, nt = case
        M, C = 37, 64
        dout, y, act = (_act(rn(M, C), dt) for _ in range(3))
        scale, mean, invstd = _stats(C, gen)
        mask = _bits(M * C, gen)
        with _bn_nt(nt):
            r = K.bn_eval_backward(d(dout), d(scale), relu_mask=d(mask) if sign == 'mask' else None,
                                   relu_act=d(act) if sign == 'act' else None, y=d(y) if params else None,
                                   running_mean=d(mean) if params else None, invstd=d(invstd) if params else None,
                                   want_params=bool(params), want_dz=bool(dz))
            torch.cuda.synchronize()
        out = {n: _sha(t) for n, t in zip(('dy', 'dz', 'dgamma', 'dbeta'), r) if t is not None}
        assert set(out) == {'dy'} | ({'dz'} if dz else set()) | ({'dgamma', 'dbeta'} if params else set())
    elif kind == 'maxpool':
        _, (N, H, W, C), dt, S = case
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dpool = _act(rn(N, Ho, Wo, C), dt)
        idx = torch.randint(0, 9, (N, Ho, Wo, C), generator=gen, dtype=torch.uint8)          # arg-max codes r * 3 + s
        y = rn(N, H, W, C)
        gamma, mean, invstd = _stats(C, gen)
        r = K.bn_backward_maxpool(d(dpool), d(idx), d(_bits(N * H * W * C, gen)), d(y), d(gamma), d(mean), d(invstd), splits=S)
        out = dict(zip(('dy', 'dgamma', 'dbeta'), map(_sha, r)))
    elif kind == 'relu_bwd':
        _, add, dt = case
        dout, a = _act(rn(37, 64), dt), _act(rn(37, 64), dt)
        out = dict(g=_sha(K.relu_bwd(d(dout), d(_bits(37 * 64, gen)), add=d(a) if add else None)))
    else:
        assert kind == 'add'
        out = dict(out=_sha(K.add(d(_act(rn(37, 64), case[1])), d(_act(rn(37, 64), case[1])))))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(_key(c) for c in CASES) and len({_key(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=_key)
def test_bn_output_bits(case, golden, dev):
    assert bn_hashes(case, dev) == golden[_key(case)]


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    table = {_key(c): bn_hashes(c, torch.device('cuda:0')) for c in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + '\n}\n')
    print('wrote', len(table), 'cases')
