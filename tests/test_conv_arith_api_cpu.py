"""Selecting the conv arithmetic through the public interface (no GPU, no library load): ``bdvcil_amd.conv_arith`` /
``get_conv_arith``, the ``conv_arith`` key of a ``CILTaskLoop`` config and ``--conv-arith`` of tools/train_cil.py."""
import importlib.util
import os

import pytest
import torch

import bdvcil_amd as bd
from bdvcil_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('bf16x3', 'f32mfma', 'bf16x2', 'f16x2', 'bf16x1', 'bf16')


def _state():
    return (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3, K.PIECES, K.ACT_DTYPE)


@pytest.fixture(autouse=True)
def _default_arith():
    """Every test starts from the default arithmetic and leaves it behind, whatever it did."""
    saved = _state()
    K.set_conv_arith('bf16x3')
    yield
    K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3, K.PIECES, K.ACT_DTYPE = saved
    K._AMAX.clear()


def test_exports():
    assert bd.conv_arith is K.conv_arith and bd.get_conv_arith is K.get_conv_arith and bd.set_conv_arith is K.set_conv_arith
    assert tuple(bd.CONV_ARITH_MODES) == MODES


@pytest.mark.parametrize('start', ['bf16x3', 'f32mfma', 'bf16'])
@pytest.mark.parametrize('mode', MODES)
def test_block_sets_the_mode_and_restores_the_globals(mode, start):
    K.set_conv_arith(start)
    before = _state()
    assert bd.get_conv_arith() == start
    with bd.conv_arith(mode) as m:
        assert m == mode and bd.get_conv_arith() == mode
        inside = _state()
    assert _state() == before and bd.get_conv_arith() == start
    K.set_conv_arith(mode)                       # the block does what the call does
    assert _state() == inside


@pytest.mark.parametrize('mode', MODES)
def test_set_conv_arith_keeps_its_return_value(mode):
    K.WGRAD_X3 = False
    assert K.set_conv_arith(mode) == (True, True, False)
    assert bd.get_conv_arith() == mode


def test_blocks_nest():
    before = _state()
    with bd.conv_arith('f16x2'):
        outer = _state()
        assert K.PIECES == K.F16X2 and K.ACT_DTYPE == torch.float32
        with bd.conv_arith('bf16'):
            assert bd.get_conv_arith() == 'bf16' and K.PIECES == 1 and K.ACT_DTYPE == torch.bfloat16
            with bd.conv_arith('f32mfma'):
                assert bd.get_conv_arith() == 'f32mfma' and not (K.FPROP_X3 or K.DGRAD_X3 or K.WGRAD_X3)
            assert bd.get_conv_arith() == 'bf16' and K.ACT_DTYPE == torch.bfloat16
        assert _state() == outer and bd.get_conv_arith() == 'f16x2'
    assert _state() == before and bd.get_conv_arith() == 'bf16x3'


@pytest.mark.parametrize('mode', MODES)
def test_restored_when_the_body_raises(mode):
    before = _state()
    with pytest.raises(RuntimeError, match='boom'):
        with bd.conv_arith('f16x2'):
            with bd.conv_arith(mode):
                raise RuntimeError('boom')
    assert _state() == before


def test_the_operand_maxima_are_dropped_on_both_edges():
    K._AMAX[1] = 'stale'
    with bd.conv_arith('f16x2'):
        assert not K._AMAX
        K._AMAX[2] = 'of the block'
    assert not K._AMAX


def test_unknown_mode_changes_nothing():
    K.set_conv_arith('bf16x2')
    before = _state()
    K._AMAX[1] = 'kept'
    with pytest.raises(ValueError, match='nope'):
        with bd.conv_arith('nope'):
            raise AssertionError('the body must not run')
    assert _state() == before and K._AMAX == {1: 'kept'}


def test_a_hand_set_state_reads_custom_and_survives_a_block():
    K.WGRAD_X3 = False
    before = _state()
    assert bd.get_conv_arith() == 'custom'
    for mode in MODES:
        with bd.conv_arith(mode):
            assert bd.get_conv_arith() == mode
        assert _state() == before and bd.get_conv_arith() == 'custom'
    K.set_conv_arith('bf16x3')
    K.ACT_DTYPE = torch.bfloat16                  # bf16 tensors without the one-product arithmetic: no mode name says that
    assert bd.get_conv_arith() == 'custom'
    K.set_conv_arith('f32mfma')
    K.PIECES = 1
    assert bd.get_conv_arith() == 'custom'


# ---- the loop's config key ---------------------------------------------------------------------------------------------

def _loop_cfg(tmp, backbone_over=None, **over):
    for name in ('train', 'val'):
        with open(tmp / f'{name}.txt', 'w') as f:
            for c in range(4):
                f.write(f'class{c}/{name}_v{c} 20 {c}\n')
    (tmp / 'rawframes').mkdir(exist_ok=True)
    backbone = dict(type='ResNetTSM', pretrained=None, depth=18, norm_eval=False, num_segments=8, shift_div=8)
    backbone.update(backbone_over or {})
    model = dict(type='CILRecognizer2D', backbone=backbone,
                 cls_head=dict(type='IncrementalTSMHead', num_classes=2, in_channels=512,
                               inc_head_config=dict(type='LocalSimilarityClassifier', out_features=2, nb_proxies=1),
                               num_segments=8, loss_cls=dict(type='LSCLoss'), spatial_type='avg',
                               consensus=dict(type='AvgConsensus', dim=1), dropout_ratio=0.5, init_std=0.001, is_shift=True),
                 train_cfg=None, test_cfg=dict(average_clips='prob'))
    cfg = dict(work_dir=str(tmp / 'work'), task_splits=[[0, 1], [2, 3]], methods='base', num_epochs_per_task=1, videos_per_gpu=2,
               budget_size=1, optimizer=dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised',
                                             paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01, momentum=0.9, weight_decay=1e-4),
               data_root=str(tmp / 'rawframes'), train_ann_file=str(tmp / 'train.txt'),
               val_ann_file=str(tmp / 'val.txt'), model=model)
    cfg.update(over)
    return cfg


def _never(*a, **kw):
    raise AssertionError('no batch is loaded at construction')


def test_check_loop_conv_arith(tmp_path):
    from bdvcil_amd.task_loop import check_loop_conv_arith
    assert check_loop_conv_arith(_loop_cfg(tmp_path)) is None
    assert check_loop_conv_arith(_loop_cfg(tmp_path, conv_arith=None)) is None
    for mode in MODES:
        assert check_loop_conv_arith(_loop_cfg(tmp_path, conv_arith=mode)) == mode
        if mode != 'bf16':                       # fp32 tensors: the eval-mode BatchNorm backward exists
            assert check_loop_conv_arith(_loop_cfg(tmp_path, dict(norm_eval=True, partial_bn=True), conv_arith=mode)) == mode
    with pytest.raises(ValueError, match='nope'):
        check_loop_conv_arith(_loop_cfg(tmp_path, conv_arith='nope'))
    for key in ('norm_eval', 'partial_bn'):
        with pytest.raises(ValueError, match=f"(?s)bf16.*{key}"):
            check_loop_conv_arith(_loop_cfg(tmp_path, {key: True}, conv_arith='bf16'))
    assert check_loop_conv_arith(_loop_cfg(tmp_path, dict(frozen_stages=1), conv_arith='bf16')) == 'bf16'


@pytest.mark.parametrize('over, backbone', [(dict(conv_arith='nope'), None), (dict(conv_arith='bf16'), dict(norm_eval=True)),
                                            (dict(conv_arith='bf16'), dict(partial_bn=True))])
def test_the_loop_refuses_at_construction(tmp_path, over, backbone):
    from bdvcil_amd.task_loop import CILTaskLoop
    before = _state()
    with pytest.raises(ValueError, match='conv_arith'):
        CILTaskLoop(_loop_cfg(tmp_path, backbone, **over), _never, device='cpu', log=lambda *a: None)
    assert not (tmp_path / 'work').exists()       # refused before anything was written
    assert _state() == before


def test_the_loop_constructs_with_frozen_stages(tmp_path):
    from bdvcil_amd.task_loop import CILTaskLoop
    before = _state()
    loop = CILTaskLoop(_loop_cfg(tmp_path, dict(frozen_stages=1), conv_arith='bf16'), _never, device='cpu', log=lambda *a: None)
    assert loop.conv_arith == 'bf16' and _state() == before
    assert CILTaskLoop(_loop_cfg(tmp_path), _never, device='cpu', log=lambda *a: None).conv_arith is None


def test_entry_points_restore_the_arithmetic_when_they_raise(tmp_path):
    """``train`` enters the loop's mode (seen by the loader, which raises on the first batch) and leaves the process's."""
    from bdvcil_amd.task_loop import CILTaskLoop
    seen = []

    def loader(infos, phase):
        seen.append(bd.get_conv_arith())
        raise RuntimeError('no frames')

    K.WGRAD_X3 = False                            # a custom state must come back exactly
    before = _state()
    loop = CILTaskLoop(_loop_cfg(tmp_path, conv_arith='f16x2'), loader, device='cpu', log=lambda *a: None)
    with pytest.raises(RuntimeError, match='no frames'):
        loop.train()
    assert seen == ['f16x2'] and _state() == before and bd.get_conv_arith() == 'custom'
    recs = loop.val_datasets[0]
    with pytest.raises(RuntimeError, match='no frames'):
        loop.predict(recs, 2)
    assert seen == ['f16x2'] * 2 and _state() == before
    with pytest.raises(FileNotFoundError):        # no checkpoint to re-test: raised inside the block as well
        loop.cil_testing()
    assert _state() == before


# ---- the command line --------------------------------------------------------------------------------------------------

def _train_cil():
    spec = importlib.util.spec_from_file_location('_train_cil_tool', os.path.join(ROOT, 'tools', 'train_cil.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag(capsys):
    tool = _train_cil()
    assert tuple(tool.CONV_ARITH_MODES) == tuple(bd.CONV_ARITH_MODES)
    ap = tool.build_parser()
    assert ap.parse_args(['cfg.py']).conv_arith is None
    for mode in MODES:
        assert ap.parse_args(['cfg.py', '--conv-arith', mode]).conv_arith == mode
    assert ap.parse_args(['cfg.py', '--conv-arith', 'f16x2', '--test']).test
    with pytest.raises(SystemExit):
        ap.parse_args(['cfg.py', '--conv-arith', 'fp8'])
    assert 'fp8' in capsys.readouterr().err
