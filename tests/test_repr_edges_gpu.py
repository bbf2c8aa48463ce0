"""Edge sweep of the evaluation and exemplar kernels -- repr / nme / class_means / herding in csrc/repr.hip, softmax_mean and topk_acc
in csrc/head_loss.hip -- against the fp64 run of oracle/repr_oracle.py (held against the fp32 oracle and the reference's goldens in
tests/test_repr_cpu.py), never against a sibling kernel.  Sizes are ragged on purpose: D below 64 and off the 64 / 256 strides, K
above 256, n below 4, B off the 4-row wave split, D = 4160 for herding's LDS request above 48 KB.

Bars
  * exact: indices, counts, zeros, NaN positions, everything on a dyadic grid (multiples of 1/8: sums of a few terms are exact);
  * a selection (herding index, NME arg-max) is compared where the fp64 margin says fp32 cannot flip it: herding inputs are drawn
    until every greedy step has a runner-up gap >= 1e-4 * max(1, largest distance); NME rows need a top-2 gap >= 1e-4;
  * herding distances 2e-6 * max(1, |dist|), class mean 2e-7 * max(1, |value|) (test_repr_gpu.py's bars, relative above 1);
  * class means: cnt * 2^-24 * max|x| per column -- an fp32 sum of cnt terms in row order, then one division;
  * repr, mean_crops (floor 2e-7) and similarity (floor 2e-6): floor + 4 x the largest deviation of the fp32 CPU oracle from the fp64
    oracle on the same case (computed from the two references only; 4 covers a wave reduction's order against ATen's);
  * softmax_mean: 1e-5 of the output scale (test_ops_gpu.py).

Largest error / bar observed on an MI355X (recorded per test with record_property):
  herding distance 0.119 ((1, 64, 1) cosine), herding class mean 0.297 ((6, 4160, 3) Euclidean), similarity 0.038 ((5, 3, 100, 257)),
  repr 0.065, mean_crops 0.102, class means 0.474 ((9, 257, 4)), softmax_mean 0.014 ((2, 10, 101)); everything else is exact.
  With the class mean summed over the rows in fp32, as herding_kernel did before this file existed, the Euclidean class mean stood at
  1.082 of its bar for (37, 96, 12) and 1.505 for (130, 320, 16) (0.844 already at six rows of D = 4160): the kernel now accumulates
  that one sum in fp64.

Herding inputs: seed 7000 + 100 * case + t, first t in range(20) that meets the margin; every case takes t = 0 except (130, 320, 16)
cosine, t = 5.

Outputs are allocated inside the wrappers; ``_poison`` (see test_pool_kernels_gpu.py) is a best effort against stale correct
values and nothing rests on it.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import repr_oracle as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff


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


# ---- herding -------------------------------------------------------------------------------------------------------------

HERDING = [(1, 64, 1), (3, 7, 3), (5, 63, 5), (6, 257, 3), (9, 100, 9), (37, 96, 12), (130, 320, 16), (6, 4160, 3)]
MARGIN = 1e-4


def _draw(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g) + 0.5 * torch.randn(1, D, generator=g)


@functools.lru_cache(maxsize=None)
def _herding_input(ci, cosine, duplicate=False):
    """(features fp32, t, fp64 reference) of the first draw whose every greedy step is decided by more than fp32 can blur."""
    n, D, m = (9, 100, 9) if duplicate else HERDING[ci]
    for t in range(20):
        f = _draw(n, D, 7000 + 100 * ci + t)
        if duplicate:
            f[5] = f[3]
        gap, far = R.herding_margin(f, m, cosine, distinct=duplicate)
        if gap >= MARGIN * max(1.0, far):
            return f, t, R.herding_select(f.double(), m, cosine)
    raise AssertionError(f'no seed in 20 gives case {ci} (cosine={cosine}) a margin of {MARGIN}')


def _check_herding(got, ref, what):
    cm, idx, dist = got
    cm64, idx64, dist64 = ref
    idx = idx.tolist() if torch.is_tensor(idx) else idx
    dist = dist.cpu() if torch.is_tensor(dist) else torch.tensor(dist, dtype=torch.float32)
    assert idx == idx64, (what, idx, idx64)
    d64 = torch.tensor(dist64, dtype=torch.float64)
    r_dist = _ratio(dist, d64, 2e-6 * d64.abs().clamp(min=1.0))
    r_cm = _ratio(cm, cm64, 2e-7 * cm64.abs().clamp(min=1.0))
    print(f'{what}: dist err/bar {r_dist:.3f}, class mean err/bar {r_cm:.3f}')
    assert r_dist <= 1.0 and r_cm <= 1.0, (what, r_dist, r_cm)
    return r_dist, r_cm


@pytest.mark.parametrize('cosine', [True, False])
@pytest.mark.parametrize('ci', range(len(HERDING)))
def test_herding_select_ragged(ci, cosine, dev, record_property):
    import bdvcil_amd as bd
    K = _k()
    n, D, m = HERDING[ci]
    f, t, ref = _herding_input(ci, cosine)
    record_property('t', t)
    fd = f.to(dev)
    _poison(dev, ((1, D), torch.float32), ((m,), torch.int64), ((m,), torch.float32))
    got = K.herding_select(fd, m, cosine)
    assert got[0].shape == (1, D) and got[1].shape == (m,) and got[1].dtype == torch.int64 and got[2].shape == (m,)
    r = _check_herding(got, ref, f'herding_select {HERDING[ci]} cosine={cosine} t={t}')
    h = bd.Herding(budget_size=m, class_indices=[0], cosine_distance=cosine, storing_methods='videos', budget_type='class')
    r2 = _check_herding(h.select(fd), ref, f'Herding.select {HERDING[ci]} cosine={cosine}')
    if m == n:
        assert sorted(got[1].tolist()) == list(range(n))                 # every row exactly once, down to the last one left
    record_property('herding dist err/bar', max(r[0], r2[0]))
    record_property('herding class mean err/bar', max(r[1], r2[1]))


@pytest.mark.parametrize('cosine', [True, False])
def test_herding_no_exemplars(cosine, dev):
    import bdvcil_amd as bd
    f, _, ref = _herding_input(2, cosine)
    cm, idx, dist = _k().herding_select(f.to(dev), 0, cosine)
    assert idx.shape == (0,) and idx.dtype == torch.int64 and dist.shape == (0,) and dist.dtype == torch.float32
    assert _ratio(cm, ref[0], 2e-7 * ref[0].abs().clamp(min=1.0)) <= 1.0         # the class mean is still produced
    cm2, idx2, dist2 = bd.Herding(0, [0], cosine, 'videos').select(f.to(dev))
    assert idx2 == [] and dist2 == []


@pytest.mark.parametrize('cosine', [True, False])
def test_herding_duplicated_row(cosine, dev, record_property):
    """Rows 3 and 5 are the same vector: their distances are bit-identical at every step, the lower index is taken first, and the
    other steps are decided by the margin to the nearest *different* distance."""
    f, t, ref = _herding_input(4, cosine, duplicate=True)
    record_property('t', t)
    assert ref[1].index(3) < ref[1].index(5)
    got = _k().herding_select(f.to(dev), 9, cosine)
    _check_herding(got, ref, f'duplicated row cosine={cosine} t={t}')
    idx = got[1].tolist()
    assert idx.index(3) < idx.index(5) and sorted(idx) == list(range(9))
    first = ref[1].index(3) + 1                                            # a budget that ends right after row 3: row 5 is never taken
    short = _k().herding_select(f.to(dev), first, cosine)[1].tolist()
    assert short == ref[1][:first] and 5 not in short


# ---- NME -----------------------------------------------------------------------------------------------------------------

NME = [(1, 1, 1, 1), (3, 2, 63, 5), (2, 1, 257, 4), (5, 3, 100, 257), (4, 10, 512, 300)]
# (first, second) class of a planted tie -> where the two sit in nme_kernel's arg-max (thread = k % 256, wave = thread / 64)
TIES = [(3, 200),       # waves 0 and 3
        (66, 130),      # waves 1 and 2, the same lane
        (67, 71),       # one wave, lanes 3 and 7
        (0, 256)]       # one thread, two trips of its k loop


def _nme_input(S, crops, D, K, seed, ties=()):
    g = torch.Generator().manual_seed(seed)
    r = F.normalize(torch.randn(S, crops, D, generator=g), dim=-1)
    means = torch.randn(K, D, generator=g)
    for row, (a, b) in enumerate(ties):
        means[b] = means[a]
        r[row] = F.normalize(means[a] + 0.1 * torch.randn(crops, D, generator=g), dim=-1)
    return r, means


def _sim_bar(r, means):
    sim64, pred64 = R.nme_classify(r.double(), means.double())
    sim32, _ = R.nme_classify(r, means)
    dev32 = torch.nan_to_num((sim32.double() - sim64).abs(), nan=0.0).max().item()
    return sim64, pred64, 2e-6 + 4 * dev32


@pytest.mark.parametrize('case', range(len(NME)))
def test_nme_ragged(case, dev, record_property):
    import bdvcil_amd as bd
    S, crops, D, K = NME[case]
    ties = TIES[:S] if K == 300 else TIES[:2] if K == 257 else ()
    r, means = _nme_input(S, crops, D, K, 8000 + case, ties)
    sim64, pred64, bar = _sim_bar(r, means)
    rd, md = r.to(dev), means.to(dev)
    _poison(dev, ((S, K), torch.float32), ((S,), torch.int64))
    sim, pred = bd.nme_classify(rd, md)
    assert sim.shape == (S, K) and pred.shape == (S,) and pred.dtype == torch.int64
    ratio = _ratio(sim, sim64, bar)
    print(f'nme {NME[case]}: bar {bar:.3e}, err/bar {ratio:.3f}')
    record_property('similarity err/bar', ratio)
    assert ratio <= 1.0
    pred = pred.cpu()
    for row, (a, b) in enumerate(ties):                # the tied pair leads by a clear margin, and the first index is returned
        rest = sim64[row].clone()
        assert rest[a] == rest[b]
        lead = rest[a].item()
        rest[[a, b]] = -float('inf')
        assert lead - rest.max().item() >= MARGIN
        assert pred64[row].item() == a and pred[row].item() == a, (row, a, b, pred[row].item())
    free = torch.arange(S) >= len(ties)
    clear = free & (R.argmax_margin(sim64) >= MARGIN)
    assert int((free & ~clear).sum()) <= S // 10       # the seeds are chosen so that the reference leaves (almost) no row undecided
    assert torch.equal(pred[clear], pred64[clear])


def test_nme_zero_and_nan_rows(dev):
    import bdvcil_amd as bd
    S, crops, D, K = 3, 2, 63, 5
    r, means = _nme_input(S, crops, D, K, 8100)
    r[1] = 0.0
    means[2] = 0.0
    sim64, pred64, bar = _sim_bar(r, means)
    sim, pred = bd.nme_classify(r.to(dev), means.to(dev))
    sim, pred = sim.cpu(), pred.cpu()
    assert torch.equal(sim[1], torch.zeros(K)) and torch.equal(sim[:, 2], torch.zeros(S))
    assert torch.equal(sim64[1], torch.zeros(K, dtype=torch.float64)) and torch.equal(sim64[:, 2], torch.zeros(S, dtype=torch.float64))
    assert _ratio(sim, sim64, bar) <= 1.0
    assert pred[1].item() == 0 == pred64[1].item()                          # all zeros: the first index
    clear = R.argmax_margin(sim64) >= MARGIN
    assert clear[0] and clear[2] and torch.equal(pred[clear], pred64[clear])
    r[1] = float('nan')
    sim64, pred64, bar = _sim_bar(r, means)
    sim, pred = bd.nme_classify(r.to(dev), means.to(dev))
    sim, pred = sim.cpu(), pred.cpu()
    assert torch.isnan(sim[1]).all() and torch.isnan(sim64[1]).all()
    assert _ratio(sim, sim64, bar) <= 1.0                                   # NaN positions agree, the other rows are untouched
    assert pred[1].item() == 0                                              # the documented deviation from torch.argmax
    assert torch.equal(pred[[0, 2]], pred64[[0, 2]])


# ---- repr ----------------------------------------------------------------------------------------------------------------

REPR = [(1, 1, 1, 1), (2, 3, 1, 63), (1, 1, 8, 257), (3, 2, 5, 300), (1, 10, 8, 4096)]


@pytest.mark.parametrize('zero_crop', [False, True])
@pytest.mark.parametrize('case', range(len(REPR)))
def test_repr_ragged(case, zero_crop, dev, record_property):
    K = _k()
    B, crops, T, D = REPR[case]
    g = torch.Generator().manual_seed(8200 + case)
    pooled = torch.randn(B * crops * T, D, generator=g)                     # signed
    if zero_crop:
        pooled.view(B, crops, T, D)[B - 1, crops - 1] = 0.0
    r64, m64 = R.predict_repr(pooled.double(), B, T)
    r32, m32 = R.predict_repr(pooled, B, T)
    bar_r = 2e-7 + 4 * (r32.double() - r64).abs().max().item()
    bar_m = 2e-7 + 4 * (m32.double() - m64).abs().max().item()
    pd = pooled.to(dev)
    _poison(dev, ((B, crops, D), torch.float32), ((B, D), torch.float32))
    r, m = K.repr_from_features(pd, B, crops, T)
    assert r.shape == (B, crops, D) and m.shape == (B, D)
    assert not torch.isnan(r).any() and not torch.isnan(m).any()
    ra, rm = _ratio(r, r64, bar_r), _ratio(m, m64, bar_m)
    print(f'repr {REPR[case]} zero_crop={zero_crop}: bars {bar_r:.3e} {bar_m:.3e}, err/bar {ra:.3f} {rm:.3f}')
    record_property('repr err/bar', ra)
    record_property('mean_crops err/bar', rm)
    assert ra <= 1.0 and rm <= 1.0
    if zero_crop:
        assert torch.equal(r[B - 1, crops - 1].cpu(), torch.zeros(D))       # 0 / max(0, 1e-12), not 0 / 0
        assert torch.equal(r64[B - 1, crops - 1], torch.zeros(D, dtype=torch.float64))
        if crops == 1:
            assert torch.equal(m[B - 1].cpu(), torch.zeros(D))


# ---- class means ---------------------------------------------------------------------------------------------------------

CLASS_MEANS = [(1, 1, 1), (5, 63, 3), (9, 257, 4), (40, 600, 7)]


def _check_class_means(x, labels, K, dev, what):
    import bdvcil_amd as bd
    n, D = x.shape
    ref = R.class_means(x.double(), labels, K)
    _poison(dev, ((K, D), torch.float32))
    got = bd.class_means_from_repr(x.to(dev), labels.to(dev), K)
    assert got.shape == (K, D)
    bar = torch.full((K, D), U, dtype=torch.float64)
    for k in range(K):
        rows = x[labels == k]
        if rows.size(0):                                                    # cnt * 2^-24 * max|x|, per column
            bar[k] = rows.size(0) * U * rows.abs().max(0).values.double()
        else:
            assert torch.isnan(ref[k]).all() and torch.isnan(got[k]).all()  # as torch.mean of nothing
    bar = bar.clamp(min=1e-300)                                             # a zero column must come out as zero: err 0 / tiny
    ratio = _ratio(got, ref, bar)
    print(f'class_means {what}: err/bar {ratio:.3f}')
    assert ratio <= 1.0
    return ratio


@pytest.mark.parametrize('case', range(len(CLASS_MEANS)))
def test_class_means_ragged(case, dev, record_property):
    n, D, K = CLASS_MEANS[case]
    g = torch.Generator().manual_seed(8300 + case)
    x = torch.randn(n, D, generator=g)
    ratios = []
    if n >= 3:
        labels = torch.arange(n) % (K - 1)              # class K - 1 stays empty
        labels[n - 2], labels[n - 1] = K + 3, -1        # two rows that belong to no class
        assert (labels == K - 1).sum() == 0
        ratios.append(_check_class_means(x, labels, K, dev, f'{CLASS_MEANS[case]}'))
        in_range = (labels >= 0) & (labels < K)
        kept = R.class_means(x[in_range].double(), labels[in_range], K)     # the out-of-range rows contribute nothing
        assert torch.equal(torch.nan_to_num(kept), torch.nan_to_num(R.class_means(x.double(), labels, K)))
    else:                                               # one row: its own class, then each out-of-range label (the class is then empty)
        for lab in (0, K + 3, -1):
            ratios.append(_check_class_means(x, torch.tensor([lab]), K, dev, f'{CLASS_MEANS[case]} label {lab}'))
    record_property('class_means err/bar', max(ratios))


# ---- top-k accuracy ------------------------------------------------------------------------------------------------------

def _dyadic(shape, g, lo=-16, hi=17):
    return torch.randint(lo, hi, shape, generator=g).float() / 8


def _plant(score, labels, b, kind):
    """Row b: kind 0 -- four classes beat the label; 1 -- five do; 2 -- nothing beats it and others tie with it; 3 -- -inf among the
    others; 4 -- the whole row is -inf.  Fewer beat it where the row is shorter."""
    K = score.shape[1]
    y = int(labels[b])
    others = [k for k in range(K) if k != y]
    if kind in (0, 1):
        beat = min(4 + kind, K - 1)
        score[b] = -1.0
        score[b, y] = 0.5
        for k in others[:beat]:
            score[b, k] = 0.5 + 0.125 * (1 + k % 3)
        for k in others[beat:beat + 2]:
            score[b, k] = 0.5                            # and two more that only tie
        return beat
    if kind == 2:
        score[b] = score[b].clamp(max=0.25)
        score[b, y] = 0.25
        for k in others[::2]:
            score[b, k] = 0.25
        return 0
    if kind == 3:
        for k in others[::3]:
            score[b, k] = -float('inf')
    else:
        score[b] = -float('inf')
    return None


@pytest.mark.parametrize('B', [1, 2, 3, 5, 9])
def test_topk_acc_counts(B, dev):
    K_ = _k()
    for Kc in (1, 4, 5, 6, 63, 64, 65, 257):
        for shift in range(5):
            g = torch.Generator().manual_seed(8400 + 10 * Kc + shift)
            score = _dyadic((B, Kc), g)
            labels = torch.randint(0, Kc, (B,), generator=g)
            if Kc > 1:
                labels[0] = (Kc - 1, 0, Kc // 2, 1, Kc - 2)[shift]           # the label at the row's ends and in its middle
            planted = [_plant(score, labels, b, (b + shift) % 5) for b in range(B)]
            sn, ln = score.numpy(), labels.numpy()
            greater = (sn > sn[np.arange(B), ln][:, None]).sum(1)
            for b, want in enumerate(planted):                               # the inputs are what they claim to be
                assert want is None or greater[b] == want, (B, Kc, shift, b)
            h1, h5 = R.topk_hit_counts(sn, ln)
            want = np.array([np.float32(h1) / np.float32(B), np.float32(h5) / np.float32(B)], dtype=np.float32)
            sd, ld = score.to(dev), labels.to(dev)
            _poison(dev, ((2,), torch.float32))
            acc = K_.topk_acc(sd, ld).cpu().numpy()
            assert acc.dtype == np.float32 and np.array_equal(acc, want), (B, Kc, shift, acc.tolist(), want.tolist(), h1, h5)


# ---- softmax mean --------------------------------------------------------------------------------------------------------

SOFTMAX = [(1, 1, 1), (3, 1, 5), (5, 3, 65), (2, 10, 101), (4, 2, 257)]


@pytest.mark.parametrize('apply_softmax', [True, False])
@pytest.mark.parametrize('case', range(len(SOFTMAX)))
def test_softmax_mean_ragged(case, apply_softmax, dev, record_property):
    K_ = _k()
    B, n, Kc = SOFTMAX[case]
    g = torch.Generator().manual_seed(8500 + case)
    exact = not apply_softmax and (n & (n - 1)) == 0
    inputs = {'dyadic': _dyadic((B * n, Kc), g)} if exact else {'randn': torch.randn(B * n, Kc, generator=g)}
    if (B, n, Kc) == (5, 3, 65):
        inputs['80 * randn'] = 80 * torch.randn(B * n, Kc, generator=g)     # expf overflows unless the row maximum is subtracted
    worst = 0.0
    for name, s in inputs.items():
        ref = R.softmax_mean(s, B, n, apply_softmax)
        assert torch.isfinite(ref).all()
        sd = s.to(dev)
        _poison(dev, ((B, Kc), torch.float32))
        out = K_.softmax_mean(sd, B, n, apply_softmax)
        assert out.shape == (B, Kc) and out.dtype == torch.float32
        if exact:
            assert torch.equal(out.cpu().double(), ref), (SOFTMAX[case], name)
            continue
        ratio = _ratio(out, ref, 1e-5 * ref.abs().max().item())
        print(f'softmax_mean {SOFTMAX[case]} apply_softmax={apply_softmax} {name}: err/bar {ratio:.3f}')
        worst = max(worst, ratio)
        assert ratio <= 1.0, (SOFTMAX[case], name, ratio)
    record_property('softmax_mean err/bar', worst)
