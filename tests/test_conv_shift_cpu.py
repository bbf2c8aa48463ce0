"""The host side of the temporal-shift sweep (tests/shift_cases.py, tests/test_conv_shift_gpu.py): the reference itself, the
preconditions of the exact regime, which kernels the cases reach, and what the plan refuses.  No GPU needed."""
import ctypes

import pytest
import torch

import shift_cases as S
from bdvcil_amd import kernels as K
from bdvcil_amd._lib import lib
from oracle.tsm_oracle import temporal_shift

BDV_EINVAL = -1


@pytest.fixture
def sweep():
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


def _roll_ref(x, T, fold):
    """The shift once more, from torch.roll over the frame axis and a mask of the frames that wrapped around a clip end."""
    n, c = x.shape[:2]
    t = torch.arange(n) % T
    ch = torch.arange(c)
    fwd, bwd = (ch < fold).view(1, c, 1, 1), ((ch >= fold) & (ch < 2 * fold)).view(1, c, 1, 1)
    nxt = torch.roll(x, -1, 0) * (t != T - 1).view(n, 1, 1, 1)
    prv = torch.roll(x, 1, 0) * (t != 0).view(n, 1, 1, 1)
    return torch.where(fwd, nxt, torch.where(bwd, prv, x))


def test_shift_ref_is_the_oracles_shift_and_the_roll_formulation():
    gen = torch.Generator().manual_seed(0)
    for clips, T, C, fold in [(c[0], c[1], c[4], c[9]) for c in S.CASES] + [(2, 8, 64, 8), (1, 1, 8, 4), (4, 3, 16, 0)]:
        x = torch.randn(clips * T, C, 2, 3, generator=gen, dtype=torch.float64)
        got = S.shift_ref(x, T, fold)
        assert got.dtype == torch.float64 and torch.equal(got, _roll_ref(x, T, fold)), (clips, T, C, fold)
        for div in range(1, C + 1):
            if fold > 0 and C // div == fold:
                assert torch.equal(got, temporal_shift(x, T, div)), (clips, T, C, fold, div)
    assert any(c[4] // 8 == c[9] for c in S.CASES) and any(c[4] % c[9] for c in S.CASES)    # both kinds of fold are in the list


def test_shift_ref_gradient_is_the_opposite_shift():
    x = torch.randn(6, 8, 1, 2, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(6, 8, 1, 2, dtype=torch.float64)
    S.shift_ref(x, 3, 4).backward(dy)
    want = dy.clone().view(2, 3, 8, 1, 2)
    d = dy.view(2, 3, 8, 1, 2)
    want[:, 1:, :4], want[:, 0, :4] = d[:, :-1, :4], 0
    want[:, :-1, 4:], want[:, -1, 4:] = d[:, 1:, 4:], 0
    assert torch.equal(x.grad, want.view(6, 8, 1, 2))


@pytest.mark.parametrize('idx', range(len(S.CASES)), ids=[S.case_id(c) for c in S.CASES])
def test_exact_regime_preconditions(idx):
    """Integers of magnitude <= 256 survive bf16 storage, sums below 2^24 survive fp32: checked on the fp64 reference alone."""
    y, dx, dw = S.exact_preconditions(idx)
    d = S.exact_data(idx)
    a = 1 if idx == len(S.CASES) - 1 else 2
    for k in ('x', 'dy', 'add', 'y_prev', 'res', 'shift'):
        assert d[k].abs().max().item() == a and torch.equal(d[k], d[k].round())
    assert set(d['w'].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert y > 0 and dx > 0 and dw > 0


def test_case_list():
    assert len(S.CASES) == 30 and len(set(S.CASES)) == 30
    assert {c[1] for c in S.CASES} == {1, 2, 3, 4, 5, 16}
    assert max(c[0] for c in S.CASES) == 43 and max(c[0] * c[1] * c[2] * c[3] for c in S.CASES) == 540
    assert {4, 12, 20, 28, 36, 60, 100} <= {c[9] for c in S.CASES}                  # fold % 8 == 4
    assert sum(2 * c[9] == c[4] for c in S.CASES) >= 4                              # no unshifted channel
    assert any(c[9] % 32 for c in S.CASES)                                          # a class boundary inside a K-step


# what conv_plan names for the cases x arithmetics x forced tiles: every family and every tile the shift is compiled into
FPROP_DGRAD_PL_TILES = ('128, 256, 2, 4, 2', '256, 128, 4, 2, 2', '256, 256, 2, 4, 1', '256, 64, 4, 2, 2', '128, 128, 2, 2, 1')
PLANNED = (
    [f'conv_{d}_kernel<128, {bn}, 2, 2>' for d in ('fprop', 'dgrad') for bn in (64, 128)]
    + [f'conv_{d}_x3_kernel<128, 128, 2, 2, true>' for d in ('fprop', 'dgrad')]
    + [f'conv_fprop_pl_kernel<{t}, {p}>' for t in FPROP_DGRAD_PL_TILES for p in (1, 2, 3)]
    + [f'conv_fprop_pl_kernel<{t}, 2, false, 4, F16Pieces>' for t in FPROP_DGRAD_PL_TILES]
    + [f'conv_dgrad_pl_kernel<{t}, {p}>' for t in FPROP_DGRAD_PL_TILES + ('64, 128, 2, 2, 1',) for p in (1, 2, 3)]
    + [f'conv_dgrad_pl_kernel<{t}, 2, 4, F16Pieces>' for t in FPROP_DGRAD_PL_TILES + ('64, 128, 2, 2, 1',)]
    + ['conv_wgrad_kernel<64, 64, 2, 2', 'conv_wgrad_kernel<128, 128, 2, 2']
    + [f'conv_wgrad_pl_kernel<{t}{f}' for t in ('128, 128', '128, 256', '256, 128', '256, 256', '64, 64', '64, 192', '256, 64', '64, 256')
       for f in ('', ', ..., F16Pieces>')])


def test_the_cases_reach_every_kernel(sweep):
    names = set()
    for mode in K.CONV_ARITH_MODES:
        for tile in S.TILES:
            sweep(mode, tile)
            for case in S.CASES:
                for d in S.DIRS:
                    plan = S.plan(case, d)
                    assert (plan is None) == S.expected_refusal(case, mode, d), (mode, tile, case, d, S.refusal(case, d))
                    if plan is not None:
                        names.add(plan.kernel.decode())
    assert len(set(PLANNED)) == len(PLANNED) == 68
    assert names == set(PLANNED), (sorted(set(PLANNED) - names), sorted(names - set(PLANNED)))


CIN32 = (9, 5, 7, 32, 128, 1, 1, 1, 0)


@pytest.mark.parametrize('fold', [0, 8])
def test_weight_gradient_of_32_input_channels_is_refused(fold, sweep):
    """No weight-gradient tile spans fewer than 64 input channels: the plan says so (it used to divide by a tile count of 0)."""
    null = ctypes.c_void_p(0)
    for mode in K.CONV_ARITH_MODES:
        sweep(mode)
        g = K.make_geom(*CIN32, 3, fold)
        g.act_dtype = 1 if mode == 'bf16' else 0
        with pytest.raises(Exception, match='Cin'):
            K.conv_plan(g, 'wgrad')
        assert K.conv_plan(g, 'fprop').kernel                   # the forward of the same site has kernels
        assert lib().bdv_conv_workspace_bytes(ctypes.byref(g), 2) == 0
    g = K.make_geom(*CIN32, 3, fold)
    for code in (lib().bdv_conv_wgrad_partial(null, null, ctypes.byref(g), null, 0, null),
                 lib().bdv_conv_wgrad(null, null, ctypes.c_void_p(16), 0.0, ctypes.byref(g), null, 0, null),
                 lib().bdv_conv_wgrad_partial_pl(null, null, ctypes.byref(g), null, 0, 3, null, null, null),
                 lib().bdv_conv_wgrad_partial_f16x2(null, null, null, null, ctypes.byref(g), null, 0, null, null, null)):
        assert code == BDV_EINVAL
        assert b'Cin=32' in lib().bdv_last_error(), lib().bdv_last_error()
    stem = K.make_geom(2, 32, 32, 4, 64, 7, 7, 2, 3)
    assert K.conv_plan(stem, 'wgrad').splits > 0 and K.conv_plan(stem, 'wgrad', x3=False).splits > 0        # Cin = 4 stays


@pytest.mark.parametrize('fold', [4, 12, 20, 36, 100])
def test_bf16_storage_refuses_a_fold_off_its_8_channel_unit(fold, sweep):
    """Under bf16 storage a thread's 16-byte unit is 8 channels and takes ONE shift class: a fold that is no multiple of 8 would
    read four channels at each class boundary from the wrong frame.  Refused in the plan, for all three directions; the same
    geometry on fp32 tensors runs (4-channel units).  Measured on the MI355X before the refusal, on the integer data of the 20
    sweep cases with fold % 8 == 4: y off by up to 4 .. 47 on every plane tile and dw by up to 15 .. 205, dx exact (the dgrad
    epilogue works in 4-channel units); every other mode and every fold % 8 == 0 case equal to fp64."""
    sweep('bf16')
    for kind in S.DIRS:
        g = K.make_geom(6, 5, 7, 256, 256, 1, 1, 1, 0, 3, fold)
        g.act_dtype = 1
        with pytest.raises(Exception, match='fold'):
            K.conv_plan(g, kind)
        g.act_dtype = 0
        sweep('bf16x1')
        assert K.conv_plan(g, kind).kernel
        sweep('bf16')
        ok = K.make_geom(6, 5, 7, 256, 256, 1, 1, 1, 0, 3, fold + 4)
        ok.act_dtype = 1
        assert K.conv_plan(ok, kind).kernel
