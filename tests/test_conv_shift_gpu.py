"""The fused temporal shift of every conv kernel, swept over clip length, fold, frame size and clip count (tests/shift_cases.py)
against the fp64 shifted convolution, in every arithmetic and under every forced plane tile.

  1. exact regime: small-integer operands, for which every bf16 / fp16 piece, product, fp32 sum and bf16-stored output is exact --
     fprop (plain, folded-BatchNorm epilogue), dgrad (plain, identity-branch add under a bit mask, fused BatchNorm-backward
     statistics), wgrad (one call; partial + batched reduce) must EQUAL fp64.  No tolerance: a channel that reads the wrong frame,
     a missing zero at a clip end or a scatter to the wrong row cannot hide behind rounding.
  2. rounded regime: randn operands (the integers have empty mid / lo pieces) under the bars the arithmetics are held to elsewhere:
     tests/test_conv_gpu.py::_close for the fp32-level modes, the definitions and bars of tests/test_bf16x2_gpu.py,
     tests/test_bf16x1_gpu.py and tests/test_bf16_storage_gpu.py::_close_to_rounding for the others, on operands pre-rounded to what
     the mode keeps (so the reference is fp64 of the operands the kernel sees).
  3. two properties: with T = 1 the shifted channels contribute nothing; the clips of a batch do not see each other.

A (mode, direction) pair is skipped only where ``conv_plan`` refuses it, and the refusals must be the expected ones
(shift_cases.expected_refusal).  Each launch is keyed by (mode, direction, kernel): a forced tile that does not apply plans the
kernel already run and is not repeated."""
import pytest
import torch

import shift_cases as S
from test_bf16_storage_gpu import _close_to_rounding
from test_bf16x1_gpu import _err, _r
from test_bf16x2_gpu import _two
from test_conv_gpu import _close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
IDS = [S.case_id(c) for c in S.CASES]


@pytest.fixture
def sweep():
    """select(mode, tile) switches the conv arithmetic and the forced plane tile; both defaults come back afterwards."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import lib
    prev = (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3)

    def select(mode, tile=-1):
        K.set_conv_arith(mode)
        assert lib().bdv_conv_debug_force_tile(tile) == 0
    try:
        yield select
    finally:
        lib().bdv_conv_debug_force_tile(-1)
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _back(t):
    """a kernel result (NHWC / OHWI, fp32 or bf16, on the device) -> fp64 NCHW / OIHW on the CPU"""
    return t.cpu().permute(0, 3, 1, 2).double()


def _launches(case, mode, select):
    """(tile, {direction: kernel name}) for every tile of the sweep: only the directions whose kernel this mode has not run yet.
    Asserts that the plan refuses exactly what shift_cases.expected_refusal names."""
    seen = set()
    for tile in (S.TILES if mode != 'f32mfma' else S.TILES[:1]):      # the fp32-MFMA kernels have one tile per column count
        select(mode, tile)
        todo = {}
        for d in S.DIRS:
            plan = S.plan(case, d)
            assert (plan is None) == S.expected_refusal(case, mode, d), (mode, tile, d, S.refusal(case, d))
            if plan is not None and (d, plan.kernel) not in seen:
                seen.add((d, plan.kernel))
                todo[d] = plan.kernel.decode()
        if todo:
            yield tile, todo


def _stats_ok(case):
    return case[7] == 1 or case[6] > 1      # a 1x1 filter with stride 2 leaves input pixels unreached: no fused statistics


@pytest.mark.parametrize('idx', range(len(S.CASES)), ids=IDS)
def test_exact(idx, dev, sweep):
    from bdvcil_amd import kernels as K
    case = S.CASES[idx]
    S.exact_preconditions(idx)
    d, ref = S.exact_data(idx), S.exact_ref(idx)
    Cin, Cout = case[4], case[5]
    g = S.geom(case)
    act = {k: _nhwc(d[k]).to(dev) for k in ('x', 'dy', 'add', 'y_prev', 'res')}
    act16 = {k: v.to(BF) for k, v in act.items()}
    w = _nhwc(d['w']).to(dev)
    ones, zeros, shift = torch.ones(Cout, device=dev), torch.zeros(Cin, device=dev), d['shift'].to(dev)
    one_in = torch.ones(Cin, device=dev)
    add_bits, relu_bits = S.pack_bits(d['add_keep']).to(dev), S.pack_bits(d['relu_keep']).to(dev)
    bad, ran = [], 0

    def check(mode, tile, kernel, what, got, want):
        if not torch.equal(got, want):
            diff = (got - want).abs()
            bad.append((mode, tile, kernel, what, f'max |diff| {diff.max().item():g} at {int((diff > 0).sum())} of {diff.numel()}'))

    for mode in K.CONV_ARITH_MODES:
        t = act16 if mode == 'bf16' else act
        for tile, todo in _launches(case, mode, sweep):
            ran += len(todo)
            if 'fprop' in todo:
                check(mode, tile, todo['fprop'], 'y', _back(K.conv_fprop(t['x'], w, g)), ref['y'])
                check(mode, tile, todo['fprop'], 'y_affine', _back(K.conv_fprop(t['x'], w, g, affine=(ones, shift, t['res'], True))),
                      ref['y_aff'])
            if 'dgrad' in todo:
                check(mode, tile, todo['dgrad'], 'dx', _back(K.conv_dgrad(t['dy'], w, g)), ref['dx'])
                dx_add = K.conv_dgrad(t['dy'], w, g, add_src=t['add'], add_mask_src=add_bits)
                check(mode, tile, todo['dgrad'], 'dx_add', _back(dx_add), ref['dx_add'])
                if _stats_ok(case):
                    dx_st, part = K.conv_dgrad(t['dy'], w, g, add_src=t['add'], add_mask_src=add_bits,
                                               bn_stats=(t['y_prev'], relu_bits, zeros, one_in))
                    assert torch.equal(dx_st, dx_add), (mode, tile, todo['dgrad'], 'dx with statistics')
                    sums = part.double().sum(1).cpu()
                    check(mode, tile, todo['dgrad'], 'sum(g)', sums[0], ref['s1'])
                    check(mode, tile, todo['dgrad'], 'sum(g * y_prev)', sums[1], ref['s2'])
            if 'wgrad' in todo:
                check(mode, tile, todo['wgrad'], 'dw', _back(K.conv_wgrad(t['dy'], t['x'], g)), ref['dw'])
                slab, dw = K.conv_wgrad_partial(t['dy'], t['x'], g)
                K.wgrad_reduce_batched([(slab, dw)])
                check(mode, tile, todo['wgrad'], 'dw (partial + reduce)', _back(dw), ref['dw'])
    print(f'[shift exact] {IDS[idx]}: {ran} (mode, direction, kernel) launches')
    assert ran >= sum(not S.expected_refusal(case, m, k) for m in K.CONV_ARITH_MODES for k in S.DIRS)
    if bad:
        pytest.fail(f'{len(bad)} results differ from fp64:\n' + '\n'.join(map(str, bad)))


def _rounded_operands(mode, x, w, dy):
    """What the mode keeps of each operand: bf16 for 'bf16x1' / 'bf16', hi + mid (16 significand bits) for 'bf16x2', else all."""
    if mode in ('bf16x1', 'bf16'):
        return _r(x), _r(w), _r(dy)
    if mode == 'bf16x2':
        return tuple(sum(_two(t)).float() for t in (x, w, dy))
    return x, w, dy


_ROUNDED_REF = {}


def _rounded_ref(idx, mode):
    """operands and fp64 (y, dx, dw) of the rounded regime, per (case, what the mode keeps); for 'bf16x2' also the mode's
    definition conv(hi + mid, hi + mid) - conv(mid, mid) (the product of the two mid pieces is not formed)."""
    keep = 'bf16' if mode in ('bf16x1', 'bf16') else 'hi+mid' if mode == 'bf16x2' else 'all'
    if (idx, keep) not in _ROUNDED_REF:
        case = S.CASES[idx]
        x, w, dy = _rounded_operands(mode, *S.rounded_data(idx))
        full = S.ref64(case, x, w, dy)
        dfn = None
        if keep == 'hi+mid':
            xm, wm, dm = (_two(t)[1] for t in (x, w, dy))
            dfn = tuple(a - b for a, b in zip(full, S.ref64(case, xm, wm, dm)))
        _ROUNDED_REF[(idx, keep)] = (x, w, dy, full, dfn)
    return _ROUNDED_REF[(idx, keep)]


@pytest.mark.parametrize('idx', range(len(S.CASES)), ids=IDS)
def test_rounded(idx, dev, sweep):
    from bdvcil_amd import kernels as K
    case = S.CASES[idx]
    g = S.geom(case)
    figures = []
    for mode in K.CONV_ARITH_MODES:
        x, w, dy, full, dfn = _rounded_ref(idx, mode)
        xd, wd, dyd = _nhwc(x).to(dev), _nhwc(w).to(dev), _nhwc(dy).to(dev)
        if mode == 'bf16':
            xd, dyd = xd.to(BF), dyd.to(BF)         # (exact: the operands are bf16 values)
        for tile, todo in _launches(case, mode, sweep):
            for k, dirn in enumerate(S.DIRS):
                if dirn not in todo:
                    continue
                out = K.conv_fprop(xd, wd, g) if k == 0 else K.conv_dgrad(dyd, wd, g) if k == 1 else K.conv_wgrad(dyd, xd, g)
                got = _back(out)
                figures.append(f'{mode} {tile} {dirn} {_err(got, full[k]):.1e}')
                where = (mode, tile, todo[dirn])
                if mode in ('bf16x3', 'f32mfma', 'f16x2'):
                    _close(got, full[k])
                elif mode == 'bf16x2':
                    if '_pl_kernel' in todo[dirn]:      # two pieces; the fp32-MFMA weight gradient (no plane tile) keeps everything
                        assert _err(got, dfn[k]) <= 2e-6, (where, _err(got, dfn[k]))
                    assert _err(got, full[k]) <= 2e-5, (where, _err(got, full[k]))
                elif mode == 'bf16x1' or dirn == 'wgrad':   # fp32 results of bf16 operands
                    assert _err(got, full[k]) <= 2e-5, (where, _err(got, full[k]))
                else:                                       # bf16-stored results
                    assert out.dtype == BF
                    _close_to_rounding(_back(out).to(BF), full[k])
    print(f'[shift rounded] {IDS[idx]}: max err / scale per (mode, tile, direction): ' + ', '.join(figures))


T1_CASES = [0, 7, 11, 14, 18, 19, 22, 24, 26, 28]


@pytest.mark.parametrize('idx', T1_CASES, ids=[IDS[i] for i in T1_CASES])
def test_a_clip_of_one_frame_zeroes_the_shifted_channels(idx, dev, sweep):
    """T = 1 (every frame its own clip, the case's integer data): both neighbours of a frame are clip ends, so y equals the
    unshifted convolution with the first 2 * fold input channels of the filter zeroed, and the first 2 * fold channels of dx hold
    what the epilogue adds (add_src under its mask) and nothing of the data gradient."""
    from bdvcil_amd import kernels as K
    clips, T, H, W, Cin, Cout, R, st, pad, fold = S.CASES[idx]
    case = (clips * T, 1, H, W, Cin, Cout, R, st, pad, fold)
    plain = case[:9] + (0,)
    d = S.exact_data(idx)
    w0 = d['w'].clone()
    w0[:, :2 * fold] = 0
    want_y = torch.nn.functional.conv2d(d['x'].double(), w0.double(), stride=st, padding=pad)
    want_add = (_nhwc(d['add']) * d['add_keep'])[..., :2 * fold].double()
    x, dy, add = _nhwc(d['x']).to(dev), _nhwc(d['dy']).to(dev), _nhwc(d['add']).to(dev)
    w, w0 = _nhwc(d['w']).to(dev), _nhwc(w0).to(dev)
    bits = S.pack_bits(d['add_keep']).to(dev)
    for mode in K.CONV_ARITH_MODES:
        sweep(mode)
        to = (lambda t: t.to(BF)) if mode == 'bf16' else (lambda t: t)
        if S.plan(case, 'fprop') is None:
            assert S.expected_refusal(case, mode, 'fprop')
            continue
        y = K.conv_fprop(to(x), w, S.geom(case))
        assert torch.equal(y, K.conv_fprop(to(x), w0, S.geom(plain))), mode
        assert torch.equal(_back(y), want_y), mode
        if S.plan(case, 'dgrad') is None:
            assert S.expected_refusal(case, mode, 'dgrad')
            continue
        dx = K.conv_dgrad(to(dy), w, S.geom(case), add_src=to(add), add_mask_src=bits)
        assert torch.equal(dx[..., :2 * fold].cpu().double(), want_add), mode
        dx0 = K.conv_dgrad(to(dy), w0, S.geom(plain), add_src=to(add), add_mask_src=bits)
        assert torch.equal(dx, dx0), mode


# fewer than four K-steps: no K split of the remainder tiles in any family, so one summation order whatever the row count
CLIP_CASES = [i for i, c in enumerate(S.CASES) if c[6] == 1 and (c[4] <= 96 or c[5] <= 96)]


@pytest.mark.parametrize('idx', CLIP_CASES, ids=[IDS[i] for i in CLIP_CASES])
def test_clips_do_not_see_each_other(idx, dev, sweep):
    """y and dx of the whole batch equal, bit for bit, the concatenation of one call per clip (randn operands), wherever both
    calls plan the same kernel and the K loop is too short to be split.  ('f16x2' scales by the maximum of the tensor it is
    given, which differs between the two calls: left to the exact regime.)"""
    from bdvcil_amd import kernels as K
    case = S.CASES[idx]
    clips, T, H, W, Cin, Cout, R, st, pad, fold = case
    x, w, dy = S.rounded_data(idx)
    xd, wd, dyd = _nhwc(x).to(dev), _nhwc(w).to(dev), _nhwc(dy).to(dev)
    g, g1 = S.geom(case), S.geom(case, clips=1)
    compared = 0
    for mode in ('bf16x3', 'f32mfma', 'bf16x2', 'bf16x1', 'bf16'):
        sweep(mode)
        to = (lambda t: t.to(BF)) if mode == 'bf16' else (lambda t: t)
        for dirn, nk, src, fn in (('fprop', Cin // 32, xd, K.conv_fprop), ('dgrad', Cout // 32, dyd, K.conv_dgrad)):
            whole, one = S.plan(case, dirn), S.plan(case, dirn, clips=1)
            if whole is None or one is None or whole.kernel != one.kernel or nk >= 4:
                continue
            got = fn(to(src), wd, g)
            per_clip = torch.cat([fn(to(c).contiguous(), wd, g1) for c in src.chunk(clips)])
            assert torch.equal(got, per_clip), (mode, dirn, whole.kernel)
            compared += 1
    assert compared > 0
