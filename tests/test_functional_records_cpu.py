"""The records the residual-block autograd nodes save through (``functional.UnitSaved`` / ``BlockSaved`` / ``BlockPlan`` /
``UnitParams``): a block flattens to 1 + 7 * n_units entries and comes back field for field, for every form a unit runs in, and
a stage's flat tensors split back into its blocks.  Host only: tiny CPU tensors, no kernel runs."""
import pytest
import torch

from bdvcil_amd import functional as Fn
from bdvcil_amd.functional import BlockPlan, BlockSaved, UnitParams, UnitSaved

FIELDS = ('y', 'act', 'mean', 'invstd', 'mask', 'scale', 'shift')


def _unit(*fields):
    """A UnitSaved with a distinct tensor in each named field and None elsewhere."""
    return UnitSaved(**{f: torch.zeros(1) for f in fields})


TRAIN = ('y', 'act', 'mean', 'invstd', 'mask')
DEFERRED = ('y', 'mean', 'invstd', 'scale', 'shift')
EVAL_LIVE = ('y', 'act', 'mean', 'invstd', 'mask', 'scale')
EVAL_FROZEN = ('act', 'scale')
DOWN_TRAIN = ('y', 'mean', 'invstd')
DOWN_LIVE = ('y', 'mean', 'invstd', 'scale')
DOWN_FROZEN = ('scale',)

BLOCKS = {
    'train BasicBlock': ([TRAIN, TRAIN], None),
    'train Bottleneck with downsample': ([TRAIN, TRAIN, TRAIN], DOWN_TRAIN),
    'Bottleneck, units 0/1 deferred': ([DEFERRED, DEFERRED, TRAIN], DOWN_TRAIN),
    'eval live/frozen/live, frozen downsample': ([EVAL_LIVE, EVAL_FROZEN, EVAL_LIVE], DOWN_FROZEN),
    'eval live/frozen/live, live downsample': ([EVAL_LIVE, EVAL_FROZEN, EVAL_LIVE], DOWN_LIVE),
}


def _block(main, down):
    return BlockSaved(torch.zeros(1), [_unit(*f) for f in main], _unit(*down) if down is not None else None)


def _assert_same_block(got, want, main, down):
    assert got.x is want.x
    assert len(got.units) == len(want.units) == len(main)
    for g, w, set_fields in list(zip(got.units, want.units, main)) + ([(got.down, want.down, down)] if down is not None else []):
        assert isinstance(g, UnitSaved)
        for f in FIELDS:
            assert getattr(g, f) is getattr(w, f), f
            assert (getattr(g, f) is not None) == (f in set_fields), f
    if down is None:
        assert got.down is None


@pytest.mark.parametrize('name', list(BLOCKS))
def test_block_saved_round_trip(name):
    main, down = BLOCKS[name]
    blk = _block(main, down)
    plan = BlockPlan([], len(main), down is not None)
    flat = blk.flatten()
    assert len(flat) == 1 + 7 * plan.n_units == plan.n_saved
    assert flat[0] is blk.x
    assert sum(t is not None for t in flat) == 1 + sum(len(f) for f in main) + len(down or ())     # nothing saved twice, nothing extra
    _assert_same_block(BlockSaved.unflatten(flat, plan.n_main, plan.has_down), blk, main, down)
    # save_for_backward hands back a tuple
    _assert_same_block(BlockSaved.unflatten(tuple(flat), plan.n_main, plan.has_down), blk, main, down)


def test_the_train_mode_downsample_keeps_no_scale_or_shift():
    main, down = BLOCKS['train Bottleneck with downsample']
    d = _block(main, down).down
    assert d.scale is None and d.shift is None and d.act is None and d.mask is None


def test_bn_stat_operands_order_and_deferred_affine():
    u = _unit(*TRAIN)
    ops = u.bn_stat_operands()
    assert len(ops) == 4 and ops[0] is u.y and ops[1] is u.mask and ops[2] is u.mean and ops[3] is u.invstd
    assert u.pre_bn is None
    v = _unit(*DEFERRED)
    assert v.pre_bn[0] is v.scale and v.pre_bn[1] is v.shift
    assert v.bn_stat_operands()[1] is None


@pytest.mark.parametrize('n_main,has_down', [(2, False), (2, True), (3, False), (3, True)])
def test_block_plan_counts(n_main, has_down):
    plan = BlockPlan([], n_main, has_down)
    assert plan.n_units == n_main + has_down
    assert plan.n_params == 3 * plan.n_units
    assert plan.n_saved == 1 + 7 * plan.n_units


def test_split_params_and_need():
    flat = [torch.zeros(1) for _ in range(9)]
    units = Fn.split_params(flat)
    assert len(units) == 3 and all(isinstance(u, UnitParams) for u in units)
    for i, u in enumerate(units):
        assert u.weight is flat[3 * i] and u.gamma is flat[3 * i + 1] and u.beta is flat[3 * i + 2]
    needs = (True, False, False, False) + (True, False, True, False, False, False)
    assert Fn.split_need(needs, 4) == [UnitParams(True, False, True), UnitParams(False, False, False)]


def test_stage_split():
    """Two blocks of different unit counts (4 and 2), flattened and followed by their parameters as ResStageFn saves them."""
    (main_a, down_a), (main_b, down_b) = BLOCKS['Bottleneck, units 0/1 deferred'], BLOCKS['train BasicBlock']
    a, b = _block(main_a, down_a), _block(main_b, down_b)
    plans = [BlockPlan(['ga'], 3, True), BlockPlan(['gb'], 2, False)]
    params = [torch.zeros(1) for _ in range(3 * (4 + 2))]
    offset = 6
    needs = (True,) + (False,) * (offset - 1) + tuple(k % 2 == 0 or k == 13 for k in range(len(params)))
    tensors = tuple(a.flatten() + b.flatten() + params)
    out = Fn.split_stage(plans, tensors, needs, offset)
    assert len(out) == 2
    p_off = 0
    for (saved, units, need), want, (main, down), plan in zip(out, (a, b), ((main_a, down_a), (main_b, down_b)), plans):
        _assert_same_block(saved, want, main, down)
        assert len(units) == len(need) == plan.n_units
        for i, (u, n) in enumerate(zip(units, need)):
            for j, f in enumerate(('weight', 'gamma', 'beta')):
                assert getattr(u, f) is params[p_off + 3 * i + j]
                assert getattr(n, f) is needs[offset + p_off + 3 * i + j]
        p_off += plan.n_params
    assert p_off == len(params)
    # one block: what ResBlockFn saves
    (saved, units, need), = Fn.split_stage(plans[1:], tuple(b.flatten() + params[:6]), (True, False, False, False) + (True,) * 6, 4)
    _assert_same_block(saved, b, main_b, down_b)
    assert units[0].weight is params[0] and units[1].weight is params[3] and need == [UnitParams(True, True, True)] * 2

