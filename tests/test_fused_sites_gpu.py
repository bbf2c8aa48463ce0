"""The FUSED forms of the conv kernels at BASELINE geometry (N = 256 frames), as every training step runs them: BatchNorm batch
statistics from the fprop epilogue (``bn_stats=True``, also behind the producer's BatchNorm applied in the loader, ``pre_bn``),
BatchNorm-backward statistics from the dgrad epilogue (``bn_stats=(y, mask, mean, invstd[, (scale, shift)])``), the stem tail
(``bn_relu_maxpool_fwd`` / ``bn_backward_maxpool``) and the standalone BatchNorm kernels at the row counts of the model.

The plain conv outputs at these sites are held to the CPU oracle by test_conv_sites_gpu.py; here the fused call must reproduce the
plain call's output bit for bit, and its side results must equal torch float64 reductions (on the GPU) of the tensors the kernels
read and wrote.  Inputs are generated on the device and conditioned as in training: conv inputs carry a per-channel offset (the
column means of y are not ~0), the producer's output has non-zero channel means, and its mask comes from bn_train_stats +
bn_apply(want_mask=True).

Statistics partials are checked twice: the column sums over all rows against the fp64 column sums (1e-5 of the column's sum of
|.|, the bar of test_fused_bn_statistics), and, where a row tile is a contiguous range of pixels (fprop; stride-1 dgrad without
temporal shift), every row against the fp64 sum of its own tile.  Each test asserts that its column bar is below a quarter of one
tile's contribution, so a lost, duplicated or stale tile cannot pass.  Measured errors are recorded as ``record_property`` pairs
'<check>' -> 'err/bar' (visible with --junitxml)."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_sites_gpu import SITES      # (tests/ is on sys.path: pytest rootdir import)

pytestmark = pytest.mark.gpu

N = 256
T = 8
EPS, MOM = 1e-5, 0.1
MODES = ('f32mfma', 'bf16x2', 'bf16x3')     # (the default last: the stem test goes on with its result)
STAT_TOL = 1e-5

NON_STEM = [s for s in SITES if s[0] != 3]
# dgrad with statistics: stride 2 needs a filter that reaches every input pixel (the 1x1 stride-2 downsample takes none)
DGRAD_STAT_SITES = [s for s in NON_STEM if not (s[2] == 1 and s[3] == 2)]
STEM = SITES[0]
# every C the BatchNorm kernels accept, at the row count of the model's sites of that width
BN_SIZES = [(802816, 64), (200704, 128), (802816, 256), (200704, 512), (50176, 1024), (12544, 2048)]


def _sid(s):
    return 'x'.join(map(str, s))


def _geom(site):
    from bdvcil_amd import kernels as K
    Cin, Cout, k, st, H, shift = site
    return K.make_geom(N, H, H, Cin, Cout, k, k, st, k // 2, T if shift else 1, Cin // 8 if shift else 0)


class _Arith:
    """K.set_conv_arith(mode) for the block's duration, restored as check_site does."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from bdvcil_amd import kernels as K
        self.prev = K.set_conv_arith(self.mode)

    def __exit__(self, *exc):
        from bdvcil_amd import kernels as K
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = self.prev


def _bar(rec, name, err, bar):
    """err <= bar (tensors: elementwise), recorded as the worst err / bar ratio."""
    if torch.is_tensor(err):
        ratio = (err / bar).max().item() if err.numel() else 0.0
    else:
        ratio = err / bar
    rec(name, f'{ratio:.3e}')
    assert ratio <= 1.0, f'{name}: worst err/bar {ratio:.3e}'


def _poison(like):
    """Best effort: hand the caching allocator a NaN-filled block of the partial's size, so that a row the kernel never writes
    shows up as non-finite (the sum checks are the guard)."""
    nan = torch.full_like(like, float('nan'))
    del nan


def _bits(mask, shape):
    """1-bit ReLU mask (int32 words, little bit order) -> bool tensor of ``shape``."""
    b = mask.view(torch.uint8)
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((b.unsqueeze(-1) >> sh) & 1).bool().reshape(shape)


def _row_tile(M, rows):
    """Rows of a row tile when ``rows`` tiles cover the M pixels in order (the planner's tiles are 64, 128 or 256 rows)."""
    fit = [bm for bm in (64, 128, 256) if -(-M // bm) == rows]
    assert len(fit) == 1, (M, rows)
    return fit[0]


def _tile_sums(v, rows):
    """(M, C) fp64 -> (rows, C) sums over consecutive row tiles."""
    M, C = v.shape
    bm = _row_tile(M, rows)
    pad = rows * bm - M
    if pad:
        v = torch.cat([v, v.new_zeros(pad, C)])
    return v.view(rows, bm, C).sum(1)


def _offset_input(gen, shape, dev):
    C = shape[-1]
    off = torch.randn(C, generator=gen, device=dev) * 0.5 + 0.3
    return torch.randn(*shape, generator=gen, device=dev) + off


def _producer(gen, shape, dev, ratio=2.0):
    """Raw output of a producing unit with non-zero channel means (|mean| / std up to ``ratio``) and its train-mode BatchNorm:
    (y, gamma, mean, invstd, scale, shift, act, mask)."""
    from bdvcil_amd import kernels as K
    C = shape[-1]
    std = torch.rand(C, generator=gen, device=dev) + 0.5
    mu = (torch.rand(C, generator=gen, device=dev) * 2 - 1) * ratio * std
    y = torch.randn(*shape, generator=gen, device=dev) * std + mu
    gamma = torch.rand(C, generator=gen, device=dev) + 0.5
    beta = torch.randn(C, generator=gen, device=dev) * 0.2
    mean, invstd, scale, shift = K.bn_train_stats(y, gamma, beta, EPS, MOM, None, None)
    act, mask = K.bn_apply(y, scale, shift, None, True, want_mask=True)
    return y, gamma, mean, invstd, scale, shift, act, mask


def _check_fprop_stats(rec, tag, y, part, tol=STAT_TOL):
    """part (2, rows, C) of a fused fprop against fp64 sums of y: every row against its tile, the columns against y's columns,
    and the column bar below a quarter of the smallest tile's sum of squares."""
    C = y.shape[-1]
    yc = y.reshape(-1, C).double()
    rows = part.shape[1]
    assert torch.isfinite(part).all(), f'{tag}: non-finite partial rows (a row the kernel never wrote)'
    p0, p1 = part[0].double(), part[1].double()
    sq = yc * yc
    # whole columns
    bar1 = tol * yc.abs().sum(0)
    bar2 = tol * sq.sum(0)
    _bar(rec, f'{tag} sum(y)', (p0.sum(0) - yc.sum(0)).abs(), bar1)
    _bar(rec, f'{tag} sum(y^2)', (p1.sum(0) - sq.sum(0)).abs(), bar2)
    # sensitivity: one tile's sum of squares is far above the column bar
    margin = (bar2 / (0.25 * p1.min(0).values)).max().item()
    rec(f'{tag} column bar / (tile sum(y^2) / 4)', f'{margin:.3e}')
    assert margin < 1.0, f'{tag}: the sum(y^2) bar does not resolve one tile ({margin:.3e})'
    # every row against its own tile
    _bar(rec, f'{tag} rows sum(y)', (p0 - _tile_sums(yc, rows)).abs(), tol * _tile_sums(yc.abs(), rows) + 1e-30)
    _bar(rec, f'{tag} rows sum(y^2)', (p1 - _tile_sums(sq, rows)).abs(), tol * _tile_sums(sq, rows) + 1e-30)


def _check_finalize(rec, tag, part, y, dev, gen):
    """bn_train_finalize(part) against a two-pass fp64 mean / variance of y (+ the running-statistics update, unbiased)."""
    from bdvcil_amd import kernels as K
    C = y.shape[-1]
    yc = y.reshape(-1, C).double()
    M = yc.shape[0]
    gamma = torch.rand(C, generator=gen, device=dev) + 0.5
    beta = torch.randn(C, generator=gen, device=dev) * 0.3
    rm0 = torch.randn(C, generator=gen, device=dev) * 0.1
    rv0 = torch.rand(C, generator=gen, device=dev) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, scale, shift = K.bn_train_finalize(part, M, gamma, beta, EPS, MOM, rm, rv)
    _check_bn_params(rec, tag, yc, mean, invstd, scale, shift, gamma, beta, rm0, rv0, rm, rv)


def _check_bn_params(rec, tag, yc, mean, invstd, scale, shift, gamma, beta, rm0, rv0, rm, rv, inv_tol=2e-5, cols=None):
    M = yc.shape[0]
    mu = yc.mean(0)
    var = (yc - mu).square().mean(0)                       # two-pass
    inv = 1.0 / (var + EPS).sqrt()
    mean, invstd, scale, shift = (t.double() for t in (mean, invstd, scale, shift))
    g64, b64 = gamma.double(), beta.double()
    sel = slice(None) if cols is None else cols
    mbar = 1e-5 * (mu.abs().max().item() + 1)
    _bar(rec, f'{tag} mean', (mean - mu)[sel].abs().max().item(), mbar)
    _bar(rec, f'{tag} invstd (rel)', ((invstd - inv).abs() / inv)[sel].max().item(), inv_tol)
    sc_ref = g64 * inv
    _bar(rec, f'{tag} scale (rel)', ((scale - sc_ref).abs() / sc_ref)[sel].max().item(), inv_tol + 1e-6)
    # shift = beta - mean * scale: the mean's error times scale plus the scale's relative error times |mean * scale|
    sh_ref = b64 - mu * sc_ref
    _bar(rec, f'{tag} shift', (shift - sh_ref)[sel].abs(), (mbar * sc_ref + (inv_tol + 1e-6) * (mu * sc_ref).abs() + 1e-6 * b64.abs())[sel])
    _bar(rec, f'{tag} running_mean', (rm.double() - ((1 - MOM) * rm0.double() + MOM * mu))[sel].abs().max().item(), MOM * mbar + 1e-6)
    rv_ref = (1 - MOM) * rv0.double() + MOM * var * M / (M - 1)
    _bar(rec, f'{tag} running_var (rel)', ((rv.double() - rv_ref).abs() / rv_ref)[sel].max().item(), 2 * inv_tol + 1e-6)


def _bn_backward_ref(g, y, mean, invstd, gamma):
    """fp64 BatchNorm backward of the masked gradient g (M, C): (dy, dgamma, dbeta, xhat)."""
    M = g.shape[0]
    xhat = (y - mean.double()) * invstd.double()
    db = g.sum(0)
    dg = (g * xhat).sum(0)
    dy = gamma.double() * invstd.double() * (g - db / M - xhat * (dg / M))
    return dy, dg, db, xhat


def _check_bn_backward(rec, tag, got, ref, tol=2e-5):
    dy, dg, db = got
    rdy, rdg, rdb = ref[:3]
    C = rdg.shape[0]
    _bar(rec, f'{tag} dy', (dy.reshape(-1, C).double() - rdy).abs().max().item(), tol * rdy.abs().max().item())
    _bar(rec, f'{tag} dgamma', (dg.double() - rdg).abs().max().item(), tol * rdg.abs().max().item())
    _bar(rec, f'{tag} dbeta', (db.double() - rdb).abs().max().item(), tol * rdb.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# 1. fused forward statistics, every non-stem site
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('site', NON_STEM, ids=_sid)
def test_fprop_bn_stats_full_size(site, mode, dev, record_property):
    from bdvcil_amd import kernels as K
    Cin, Cout, k, st, H, shift = site
    gen = torch.Generator(device=dev).manual_seed(7000 + Cin + 7 * Cout + k + st)
    x = _offset_input(gen, (N, H, H, Cin), dev)
    w = torch.randn(Cout, k, k, Cin, generator=gen, device=dev) / (Cin * k * k) ** 0.5
    with _Arith(mode):
        g = _geom(site)
        y0 = K.conv_fprop(x, w, g)
        y, part = K.conv_fprop(x, w, g, bn_stats=True)
        assert torch.equal(y, y0)
        y2 = torch.empty_like(y)
        _poison(part)
        y2, part2 = K.conv_fprop(x, w, g, out=y2, bn_stats=True)
        assert torch.equal(y2, y0) and torch.equal(part2, part), 'fused fprop statistics are not reproducible (unwritten rows?)'
        del y2, part2
        _check_fprop_stats(record_property, 'fprop', y, part)
        _check_finalize(record_property, 'finalize', part, y, dev, gen)
        if not K.fprop_pre_ok(g):
            return
        # the consumer of a producer whose BatchNorm + ReLU is applied in this conv's loaders (conv3 / downsample geometry)
        del y, y0, part
        yp, _, _, _, scale, shift, act, _ = _producer(gen, (N, H, H, Cin), dev)
        ya = K.conv_fprop(act, w, g)
        yq0 = K.conv_fprop(yp, w, g, pre_bn=(scale, shift))
        yq, pq = K.conv_fprop(yp, w, g, bn_stats=True, pre_bn=(scale, shift))
        assert torch.equal(yq, yq0)
        _bar(record_property, 'pre_bn y vs conv(bn_apply)', (yq - ya).abs().max().item(), 2e-6 * ya.abs().max().item())
        del ya, yq0
        _check_fprop_stats(record_property, 'pre_bn fprop', yq, pq)
        _check_finalize(record_property, 'pre_bn finalize', pq, yq, dev, gen)
        dy = torch.randn(N, g.Ho, g.Wo, Cout, generator=gen, device=dev)
        assert torch.equal(K.conv_wgrad(dy, yp, g, pre_bn=(scale, shift)), K.conv_wgrad(dy, act, g))


# ---------------------------------------------------------------------------------------------------------------------
# 2. fused BatchNorm-backward statistics of the dgrad epilogue
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('site', DGRAD_STAT_SITES, ids=_sid)
def test_dgrad_bn_stats_full_size(site, mode, dev, record_property):
    from bdvcil_amd import kernels as K
    Cin, Cout, k, st, H, shift = site
    gen = torch.Generator(device=dev).manual_seed(8000 + Cin + 7 * Cout + k + st)
    w = torch.randn(Cout, k, k, Cin, generator=gen, device=dev) / (Cout * k * k) ** 0.5
    rec = record_property
    with _Arith(mode):
        g = _geom(site)
        yp, gamma, mean, invstd, scale, shift_, _, mask = _producer(gen, (N, H, H, Cin), dev)
        dy = _offset_input(gen, (N, g.Ho, g.Wo, Cout), dev)
        add = amask = None
        if shift:       # conv1 of a block: residual gradient and the block output's ReLU mask in the epilogue
            add = torch.randn(N, H, H, Cin, generator=gen, device=dev)
            amask = torch.randint(-2 ** 31, 2 ** 31 - 1, (N * H * H * Cin // 32,), generator=gen, device=dev,
                                  dtype=torch.int64).to(torch.int32)
        dx0 = K.conv_dgrad(dy, w, g, add_src=add, add_mask_src=amask)
        dx, part = K.conv_dgrad(dy, w, g, add_src=add, add_mask_src=amask, bn_stats=(yp, mask, mean, invstd))
        assert torch.equal(dx, dx0)
        dx2 = torch.empty_like(dx)
        _poison(part)
        dx2, part2 = K.conv_dgrad(dy, w, g, add_src=add, add_mask_src=amask, out=dx2, bn_stats=(yp, mask, mean, invstd))
        assert torch.equal(dx2, dx0) and torch.equal(part2, part), 'fused dgrad statistics are not reproducible (unwritten rows?)'
        del dx0, dx2, part2
        assert torch.isfinite(part).all()
        M = N * H * H
        gm = dx.reshape(M, Cin).double() * _bits(mask, (M, Cin))
        rdy, rdg, rdb, xhat = _bn_backward_ref(gm, yp.reshape(M, Cin).double(), mean, invstd, gamma)
        gx = gm * xhat
        rows = part.shape[1]
        p0, p1 = part[0].double(), part[1].double()
        bar0, bar1 = STAT_TOL * gm.abs().sum(0), STAT_TOL * gx.abs().sum(0)
        _bar(rec, 'dgrad sum(g)', (p0.sum(0) - rdb).abs(), bar0)
        _bar(rec, 'dgrad sum(g xhat)', (p1.sum(0) - rdg).abs(), bar1)
        if st == 1 and not shift:     # row tiles are contiguous pixel ranges: every row against its own tile
            tabs = _tile_sums(gx.abs(), rows)
            _bar(rec, 'dgrad rows sum(g)', (p0 - _tile_sums(gm, rows)).abs(), STAT_TOL * _tile_sums(gm.abs(), rows) + 1e-30)
            _bar(rec, 'dgrad rows sum(g xhat)', (p1 - _tile_sums(gx, rows)).abs(), STAT_TOL * tabs + 1e-30)
        else:                         # (temporal scatter / parity classes) an average tile
            tabs = gx.abs().sum(0, keepdim=True) / rows
        margin = (bar1 / (0.25 * tabs.min(0).values)).max().item()
        rec('dgrad column bar / (tile sum|g xhat| / 4)', f'{margin:.3e}')
        assert margin < 1.0, f'the sum(g xhat) bar does not resolve one tile ({margin:.3e})'
        del gx
        # the producer's apply pass skipped (its consumer takes pre_bn): the ReLU sign derived from y
        if K.fprop_pre_ok(g):
            dxd, partd = K.conv_dgrad(dy, w, g, add_src=add, add_mask_src=amask, bn_stats=(yp, None, mean, invstd, (scale, shift_)))
            assert torch.equal(dxd, dx) and torch.equal(partd, part)
            del dxd, partd
        ref = (rdy, rdg, rdb)
        got = K.bn_backward(dx, mask, yp, gamma, mean, invstd, True, stat_partial=part)
        _check_bn_backward(rec, 'bn_backward(stat_partial)', got, ref)
        alone = K.bn_backward(dx, mask, yp, gamma, mean, invstd, True)
        for name, u, v in zip(('dy', 'dgamma', 'dbeta'), got, alone):
            _bar(rec, f'stat_partial vs standalone {name}', (u - v).abs().max().item(), 2e-5 * v.abs().max().item())
        if K.fprop_pre_ok(g):
            derived = K.bn_backward(dx, None, yp, gamma, mean, invstd, True, stat_partial=part, relu_affine=(scale, shift_))
            for u, v in zip(got, derived):
                assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the stem at full size: 224^2 -> 112^2 x 64 -> 56^2
# ---------------------------------------------------------------------------------------------------------------------
def test_stem_fused_full_size(dev, record_property):
    from bdvcil_amd import kernels as K
    Cin, Cout, k, st, H, _ = STEM
    rec = record_property
    gen = torch.Generator(device=dev).manual_seed(9000)
    x4 = _offset_input(gen, (N, H, H, 4), dev)
    x4[..., 3] = 0
    w4 = torch.randn(Cout, k, k, 4, generator=gen, device=dev) / (Cin * k * k) ** 0.5
    w4[..., 3] = 0
    g = K.make_geom(N, H, H, 4, Cout, k, k, st, k // 2)
    for mode in MODES:
        with _Arith(mode):
            y0 = K.conv_fprop(x4, w4, g)
            y, part = K.conv_fprop(x4, w4, g, bn_stats=True)
            assert torch.equal(y, y0)
            del y0
            # 25 088 row tiles of 128 pixels: 1e-5 of a column is a quarter of one tile's sum; 2e-6 keeps the one-tile margin
            # (an fp32 tile sum of 128 terms is good to ~1e-7 of its sum of |.|; the fp64 finalize adds nothing)
            _check_fprop_stats(rec, f'stem fprop {mode}', y, part, tol=2e-6)
    del x4                      # (y, part of the default arithmetic, the last one run, go on)
    gamma = torch.rand(Cout, generator=gen, device=dev) + 0.5
    beta = torch.randn(Cout, generator=gen, device=dev) * 0.3
    M = y.numel() // Cout
    mean, invstd, scale, shift = K.bn_train_finalize(part, M, gamma, beta, EPS, MOM, None, None)
    _check_finalize(rec, 'stem finalize', part, y, dev, gen)
    del part
    # BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one pass
    p, idx, mask = K.bn_relu_maxpool_fwd(y, scale, shift)
    a = torch.relu(y.double() * scale.double() + shift.double())
    pref = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    ulp = torch.nextafter(pref.float(), torch.tensor(float('inf'), device=dev)).double() - pref.float().double()
    _bar(rec, 'stem pooled (fp32 ulps)', ((p.double() - pref).abs() / ulp).max().item(), 1.0)
    assert torch.equal(_bits(mask, a.shape), a > 0)
    del pref
    # the arg-max codes point at a window element within one ulp of the window's maximum
    Ho = p.shape[1]
    t = idx.long()
    assert (t <= 8).all()
    ar = torch.arange(Ho, device=dev)
    hi = 2 * ar.view(1, Ho, 1, 1) - 1 + t // 3
    wi = 2 * ar.view(1, 1, Ho, 1) - 1 + t % 3
    assert ((hi >= 0) & (hi < a.shape[1]) & (wi >= 0) & (wi < a.shape[2])).all()
    nn_ = torch.arange(N, device=dev).view(N, 1, 1, 1).expand_as(t)
    cc = torch.arange(Cout, device=dev).view(1, 1, 1, Cout).expand_as(t)
    assert (a[nn_, hi, wi, cc] >= p.double() - ulp).all()
    del t, ulp
    # backward behind the max-pool: fp64 max_unpool (at the arg-max the kernel chose) + ReLU mask + BatchNorm backward
    dp = torch.randn(p.shape, generator=gen, device=dev)
    da = torch.zeros_like(a)
    da.index_put_((nn_, hi, wi, cc), dp.double(), accumulate=True)
    del nn_, hi, wi, cc
    gm = (da * (a > 0)).reshape(M, Cout)
    del da, a
    ref = _bn_backward_ref(gm, y.reshape(M, Cout).double(), mean, invstd, gamma)
    got = K.bn_backward_maxpool(dp, idx, mask, y, gamma, mean, invstd)
    _check_bn_backward(rec, 'stem bn_backward_maxpool', got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 4. standalone BatchNorm kernels at production row counts (bn_grid's row-block cap binds)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,C', BN_SIZES, ids=lambda v: str(v))
def test_bn_kernels_production_rows(M, C, dev, record_property):
    from bdvcil_amd import kernels as K
    rec = record_property
    gen = torch.Generator(device=dev).manual_seed(M + C)
    std = torch.rand(C, generator=gen, device=dev) + 0.5
    mu = (torch.rand(C, generator=gen, device=dev) * 6 - 3) * std         # |mean| / std <= 3
    y = torch.randn(M, C, generator=gen, device=dev) * std + mu
    gamma = torch.rand(C, generator=gen, device=dev) + 0.5
    beta = torch.randn(C, generator=gen, device=dev) * 0.3
    rm0 = torch.randn(C, generator=gen, device=dev) * 0.1
    rv0 = torch.rand(C, generator=gen, device=dev) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, scale, shift = K.bn_train_stats(y, gamma, beta, EPS, MOM, rm, rv)
    yc = y.double()
    _check_bn_params(rec, 'bn_train_stats', yc, mean, invstd, scale, shift, gamma, beta, rm0, rv0, rm, rv)
    # apply with a residual and the ReLU mask: one fused multiply-add, one add
    res = torch.randn(M, C, generator=gen, device=dev)
    out, mask = K.bn_apply(y, scale, shift, res, True, want_mask=True)
    oref = torch.relu(yc * scale.double() + shift.double() + res.double())
    _bar(rec, 'bn_apply', (out.double() - oref).abs().max().item(), 2e-6 * oref.abs().max().item())
    assert torch.equal(_bits(mask, (M, C)), out > 0)
    del res, oref
    dout = torch.randn(M, C, generator=gen, device=dev)
    gm = dout.double() * (out > 0)
    del out
    ref = _bn_backward_ref(gm, yc, mean, invstd, gamma)
    _check_bn_backward(rec, 'bn_backward', K.bn_backward(dout, mask, y, gamma, mean, invstd, True), ref)


def test_bn_train_stats_conditioned(dev, record_property):
    """Channels with |mean| / std = 30 (asserted: invstd to 1e-4), 100 and 300 (recorded only: the variance is formed one-pass
    as E[y^2] - E[y]^2 in the finalize)."""
    from bdvcil_amd import kernels as K
    M, C = 802816, 64
    gen = torch.Generator(device=dev).manual_seed(31)
    ratio = torch.full((C,), 1.0, device=dev)
    ratio[0], ratio[1], ratio[2] = 30.0, 100.0, 300.0
    y = torch.randn(M, C, generator=gen, device=dev) + ratio
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    mean, invstd, _, _ = K.bn_train_stats(y, gamma, beta, EPS, MOM, None, None)
    yc = y.double()
    mu = yc.mean(0)
    inv = 1.0 / ((yc - mu).square().mean(0) + EPS).sqrt()
    rel = (invstd.double() - inv).abs() / inv
    for c, r in ((1, 100), (2, 300)):
        record_property(f'invstd (rel) at |mean|/std = {r}', f'{rel[c].item():.3e}')
    _bar(record_property, 'invstd (rel) at |mean|/std = 30', rel[0].item(), 1e-4)
    _bar(record_property, 'invstd (rel) at |mean|/std <= 1', rel[3:].max().item(), 2e-5)
    _bar(record_property, 'mean at |mean|/std = 30', (mean.double() - mu)[0].abs().item(), 1e-5 * (mu.abs().max().item() + 1))
