"""CPU tests of the representation-path oracle (oracle/repr_oracle.py): the herding restatement is pinned against
golden vectors produced by the reference's own Herding.construct_exemplar (tests/golden/make_golden_herding.py);
the cil.py snippets (predict_step representation, NME, class means) are checked at definition level.  The fp64 run of the same
functions, the margin helpers and the argument refusals of csrc/repr.hip's entry points (no launch, no GPU) follow."""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import repr_oracle as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'herding_golden.npz')
N_CASES = 7


def _t(a):
    return torch.from_numpy(np.asarray(a))


def iter_golden_classes():
    gz = np.load(GOLD)
    for ci in range(N_CASES):
        clips, cosine, ncls, budget = [int(v) for v in gz[f'c{ci}_cfg']]
        feats, labels = _t(gz[f'c{ci}_feats']), _t(gz[f'c{ci}_labels'])
        for c in range(ncls):
            sel = feats[(labels == c).nonzero(as_tuple=True)[0]]
            yield dict(case=ci, cls=c, method='clips' if clips else 'videos', cosine=bool(cosine), budget=budget, feats=sel,
                       indices=gz[f'c{ci}_k{c}_indices'].tolist(), dist=_t(gz[f'c{ci}_k{c}_dist']),
                       class_mean=_t(gz[f'c{ci}_k{c}_class_mean']))


def test_herding_oracle_matches_reference_golden():
    n = 0
    for g in iter_golden_classes():
        f = R.herding_class_features(g['feats'], g['method'])
        cm, idx, dist = R.herding_select(f, g['budget'], g['cosine'])
        assert idx == g['indices'], (g['case'], g['cls'])
        assert torch.allclose(torch.tensor(dist), g['dist'], rtol=0, atol=1e-6)
        assert torch.allclose(cm, g['class_mean'], rtol=0, atol=1e-7)
        assert len(set(idx)) == len(idx) == g['budget']
        n += 1
    assert n == 17


def test_golden_has_an_exact_tie_and_a_full_class():
    cases = list(iter_golden_classes())
    full = [g for g in cases if g['case'] == 6]
    assert all(sorted(g['indices']) == list(range(8)) for g in full)        # every sample of the class gets picked
    assert any(g['case'] == 2 for g in cases)


def test_predict_repr_definition():
    g = torch.Generator().manual_seed(0)
    B, crops, T, D = 3, 2, 8, 32
    pooled = torch.randn(B * crops * T, D, 1, 1, generator=g)
    r, m = R.predict_repr(pooled, B, T)
    assert r.shape == (B, crops, D) and m.shape == (B, D)
    ref = pooled.flatten(1).view(B, crops, T, D).mean(2)
    ref = ref / ref.norm(dim=-1, keepdim=True)
    assert torch.allclose(r, ref, atol=1e-6)
    assert torch.allclose(m, ref.mean(1), atol=1e-6)


def test_nme_and_class_means_definition():
    g = torch.Generator().manual_seed(1)
    S, crops, D, K = 9, 3, 16, 5
    r = F.normalize(torch.randn(S, crops, D, generator=g), dim=-1)
    means = torch.randn(K, D, generator=g)
    sim, pred = R.nme_classify(r, means)
    ref = torch.einsum('scd,kd->sck', r, F.normalize(means, dim=-1)).mean(1)
    assert torch.allclose(sim, ref, atol=1e-6) and torch.equal(pred, ref.argmax(1))
    labels = torch.tensor([0, 1, 2, 0, 1, 2, 4, 4, 0])
    cm = R.class_means(r.mean(1), labels, K)
    assert torch.allclose(cm[4], r.mean(1)[6:8].mean(0), atol=1e-7)
    assert torch.isnan(cm[3]).all()                                          # empty class: mean of nothing


# ---- the fp64 side of the oracle (what tests/test_repr_edges_gpu.py holds the kernels against) ----------------------------

def test_oracle_computes_in_the_dtype_of_its_inputs():
    g = torch.Generator().manual_seed(2)
    B, crops, T, D, K = 2, 3, 4, 10, 5
    pooled = torch.randn(B * crops * T, D, generator=g, dtype=torch.float64)
    r, m = R.predict_repr(pooled, B, T)
    means = torch.randn(K, D, generator=g, dtype=torch.float64)
    sim, pred = R.nme_classify(r, means)
    cm = R.class_means(m, torch.tensor([0, 3]), K)
    hm, idx, dist, steps = R.herding_trace(pooled[:7], 7, True)
    he = R.herding_select(pooled[:7], 3, False)[0]
    for t in (r, m, sim, cm, hm, he, steps[0]):
        assert t.dtype == torch.float64
    assert pred.dtype == torch.int64 and sorted(idx) == list(range(7))
    r32, m32 = R.predict_repr(pooled.float(), B, T)
    assert r32.dtype == torch.float32 and (r32.double() - r).abs().max() < 1e-6
    assert R.herding_select(pooled[:7].float(), 3, True)[0].dtype == torch.float32


def test_fp64_herding_agrees_with_the_fp32_oracle_on_the_goldens():
    """Same indices; distances and class means within this module's bars (1e-6 / 1e-7, test_herding_oracle_matches_reference_golden)."""
    n = 0
    for g in iter_golden_classes():
        f = R.herding_class_features(g['feats'], g['method'])
        cm32, idx32, dist32 = R.herding_select(f, g['budget'], g['cosine'])
        cm64, idx64, dist64 = R.herding_select(f.double(), g['budget'], g['cosine'])
        assert cm64.dtype == torch.float64
        assert idx64 == idx32 == g['indices'], (g['case'], g['cls'])
        assert torch.allclose(torch.tensor(dist64, dtype=torch.float64), torch.tensor(dist32, dtype=torch.float64), rtol=0, atol=1e-6)
        assert torch.allclose(torch.tensor(dist64, dtype=torch.float64), g['dist'].double(), rtol=0, atol=1e-6)
        if not g['cosine']:          # an fp32 sum of rows values, then one division: at most rows * 2^-24 * max|x| from the exact mean
            assert ((cm64 - cm32.double()).abs() <= f.size(0) * 2.0 ** -24 * f.abs().max(0, keepdim=True).values.double()).all()
        else:                        # v = mean / |mean|: an element error e of the mean moves v by at most e / |mean| directly and by
            e = f.size(0) * 2.0 ** -24 * f.abs().max().item()     # |v| sqrt(D) e / |mean| through the norm; two roundings of the division
            bound = e / f.double().mean(0).norm().item() * (1 + f.size(1) ** 0.5) + 2.0 ** -23
            assert (cm64 - cm32.double()).abs().max().item() <= bound
        n += 1
    assert n == 17


def test_margins_and_the_two_evaluation_restatements():
    f = torch.tensor([[0., 0.], [1., 0.], [1., 0.], [5., 5.]])
    gap, far = R.herding_margin(f, 4, False)
    assert gap == 0.0                                                        # rows 1 and 2 are the same point
    gap_d, far_d = R.herding_margin(f, 4, False, distinct=True)
    assert gap_d > 0.1 and far_d == far > 0
    assert R.herding_margin(f[:1], 1, True) == (float('inf'), R.herding_select(f[:1].double(), 1, True)[2][0])
    assert R.herding_margin(f, 0, True) == (float('inf'), 0.0)
    m = R.argmax_margin(torch.tensor([[1., 3., 2.5], [4., 4., 0.]], dtype=torch.float64))
    assert m.tolist() == [0.5, 0.0] and R.argmax_margin(torch.zeros(2, 1)).tolist() == [float('inf')] * 2
    s = torch.tensor([[0., 0.], [2., 0.], [1., 1.], [1., 3.]])
    assert torch.equal(R.softmax_mean(s, 2, 2, False), torch.tensor([[1., 0.], [1., 2.]], dtype=torch.float64))
    sm = R.softmax_mean(80 * s, 2, 2, True)
    assert sm.dtype == torch.float64 and torch.isfinite(sm).all() and torch.allclose(sm.sum(1), torch.ones(2, dtype=torch.float64))
    score = np.array([[1., 2., 3., 4., 5., 6.], [1., 1., 0., 0., 0., 0.], [6., 5., 4., 3., 2., 1.], [-np.inf] * 6], dtype=np.float32)
    assert R.topk_hit_counts(score, np.array([0, 1, 0, 2])) == (3, 3)        # 5 beat it; tied, not beaten; best; all -inf
    assert R.topk_hit_counts(score, np.array([1, 2, 1, 0])) == (1, 4)        # 4 beat it; 2 beat it; 1 beats it; all -inf


# ---- host-side refusals of csrc/repr.hip: every call below fails on its arguments before any launch ---------------------------

def _lib():
    import bdvcil_amd as bd
    return bd._lib.lib()


ONE = ctypes.c_void_p(16)         # never dereferenced


def _refused(rc, name, code=-1):
    msg = _lib().bdv_last_error()
    assert rc == code and msg.startswith(name.encode() + b':'), (rc, msg)
    return msg


def test_herding_select_refusals():
    lib = _lib()
    ws = 1 << 30

    def call(n, D, m, ws_ptr=ONE, ws_bytes=ws, feat=ONE):
        return lib.bdv_herding_select(feat, n, D, m, 0, ONE, ONE, ONE, ws_ptr, ws_bytes, None)

    assert b'9 exemplars requested from 8' in _refused(call(8, 64, 9), 'bdv_herding_select')
    assert b'-1 exemplars' in _refused(call(8, 64, -1), 'bdv_herding_select')
    assert b'D=8193' in _refused(call(8, 8193, 4), 'bdv_herding_select')
    for n, D in ((0, 64), (-3, 64), (8, 0), (8, -1)):
        assert b'bad argument' in _refused(call(n, D, 0), 'bdv_herding_select')
    assert b'bad argument' in _refused(call(8, 64, 4, feat=None), 'bdv_herding_select')
    assert b'bad argument' in _refused(call(8, 64, 4, ws_ptr=None), 'bdv_herding_select')
    for n, D in ((8, 64), (5, 63), (3, 8192)):
        need = lib.bdv_herding_workspace_bytes(n, D)
        msg = _refused(call(n, D, n, ws_bytes=need - 1), 'bdv_herding_select', code=-2)
        assert b'workspace %d < required %d' % (need - 1, need) in msg


def test_nme_classify_refusals():
    lib = _lib()

    def call(S, crops, D, K, ws_bytes=1 << 30, ws_ptr=ONE):
        return lib.bdv_nme_classify(ONE, ONE, ONE, ONE, S, crops, D, K, ws_ptr, ws_bytes, None)

    assert b'D + K = 16385' in _refused(call(4, 2, 16000, 385), 'bdv_nme_classify')
    assert b'D + K = 16385' in _refused(call(4, 2, 1, 16384), 'bdv_nme_classify')
    for bad in ((0, 2, 64, 5), (4, 0, 64, 5), (4, 2, 0, 5), (4, 2, 64, 0), (-1, 2, 64, 5), (4, 2, 64, -5)):
        assert b'bad argument' in _refused(call(*bad), 'bdv_nme_classify')
    assert b'bad argument' in _refused(call(4, 2, 64, 5, ws_ptr=None), 'bdv_nme_classify')
    for K, D in ((5, 64), (257, 100), (384, 16000)):
        need = lib.bdv_nme_workspace_bytes(K, D)
        msg = _refused(call(4, 2, D, K, ws_bytes=need - 1), 'bdv_nme_classify', code=-2)
        assert b'workspace %d < required %d' % (need - 1, need) in msg


def test_repr_from_features_refusals():
    lib = _lib()

    def call(B, crops, T, D, feat=ONE):
        return lib.bdv_repr_from_features(feat, ONE, ONE, B, crops, T, D, None)

    assert b'D=4097' in _refused(call(2, 3, 8, 4097), 'bdv_repr_from_features')
    for bad in ((0, 3, 8, 64), (2, 0, 8, 64), (2, 3, 0, 64), (2, 3, 8, 0), (2, -3, 8, 64)):
        assert b'bad argument' in _refused(call(*bad), 'bdv_repr_from_features')
    assert b'bad argument' in _refused(call(2, 3, 8, 64, feat=None), 'bdv_repr_from_features')


def test_workspace_size_functions():
    lib = _lib()
    for n, D in ((1, 1), (3, 7), (4, 64), (5, 63), (130, 320), (6, 4160), (1000, 8192)):
        assert lib.bdv_herding_workspace_bytes(n, D) == n * D * 4 + (n * 4 + 15) // 16 * 16
    for K, D in ((1, 1), (5, 63), (257, 100), (300, 512), (384, 16000)):
        assert lib.bdv_nme_workspace_bytes(K, D) == K * D * 4
    for a, b in ((0, 64), (64, 0), (-1, 64), (64, -1), (0, 0)):
        assert lib.bdv_herding_workspace_bytes(a, b) == 0 and lib.bdv_nme_workspace_bytes(a, b) == 0
