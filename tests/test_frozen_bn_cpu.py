"""``norm_eval`` / ``frozen_stages`` / ``partial_bn`` on the host: module flags and ``requires_grad`` after every way of switching
modes (UPSTREAM ``ResNet.train`` re-applies the options on each call), the constructor signatures, and the new entry point
``bdv_bn_eval_backward`` in the header, the ctypes table and the built library."""
import ctypes
import inspect
import os
import re

import pytest
import torch.nn as nn

import bdvcil_amd as bd
from bdvcil_amd.resnet3d import ResNet3d
from bdvcil_amd.resnet_tsm import ResNetTSM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN = (nn.BatchNorm2d, nn.BatchNorm3d)


def _bns(m):
    return [(n, b) for n, b in m.named_modules() if isinstance(b, BN)]


def _stage_of(name):
    """0 = the stem, 1..4 = layerN."""
    return 0 if name.startswith('conv1') else int(name[5])


def _check(m, mode, frozen_stages=-1, norm_eval=False, partial_bn=False, all_unfrozen=False):
    """Flags of ``m`` after ``m.train(mode)`` under the given options; ``all_unfrozen``: unfreeze_backbone() ran since, and no
    train() call after it (requires_grad is True everywhere, module modes as left by the last train())."""
    for k, (name, b) in enumerate(_bns(m)):
        frozen = _stage_of(name) <= frozen_stages
        want_train = mode and not frozen and not norm_eval and not (partial_bn and k >= 1)
        assert b.training == want_train, (name, b.training, want_train)
        affine_frozen = (frozen or (mode and partial_bn and k >= 1)) and not all_unfrozen
        assert b.weight.requires_grad == (not affine_frozen), name
        assert b.bias.requires_grad == (not affine_frozen), name
    for name, p in m.named_parameters():
        if 'bn' not in name.split('.'):
            assert p.requires_grad == (all_unfrozen or _stage_of(name) > frozen_stages), name
    # non-BatchNorm modules follow train(mode), frozen stages stay in eval
    for li in range(1, 5):
        assert getattr(m, f'layer{li}').training == (mode and li > frozen_stages)


OPTIONS = [dict(), dict(norm_eval=True), dict(partial_bn=True), dict(frozen_stages=0), dict(frozen_stages=1), dict(frozen_stages=4),
           dict(frozen_stages=1, norm_eval=True), dict(frozen_stages=2, partial_bn=True), dict(norm_eval=True, partial_bn=True)]


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: ','.join(f'{k}={v}' for k, v in o.items()) or 'default')
def test_tsm_flags_after_train_eval_and_unfreeze(opts):
    m = ResNetTSM(18, **opts)
    m.init_weights()
    m.train()
    _check(m, True, **opts)
    m.eval()
    # eval(): every BatchNorm in eval; partial_bn froze the affine in the train() call before and nothing un-freezes it
    for k, (name, b) in enumerate(_bns(m)):
        assert not b.training
        frozen = _stage_of(name) <= opts.get('frozen_stages', -1) or (opts.get('partial_bn', False) and k >= 1)
        assert b.weight.requires_grad == (not frozen), name
    m.train()
    _check(m, True, **opts)
    # freeze_backbone() / unfreeze_backbone() of the recognizer touch requires_grad only; the next train() restores the options
    for p in m.parameters():
        p.requires_grad = False
    for p in m.parameters():
        p.requires_grad = True
    _check(m, True, all_unfrozen=True, **opts)
    m.train()
    _check(m, True, **opts)


def test_recognizer_unfreeze_then_train_restores_the_options():
    from oracle import tsm_oracle as O
    cfg = O.r50_cfg(num_classes=5, depth=18, dropout_ratio=0.0)
    cfg['backbone'].update(frozen_stages=1, partial_bn=True)
    m = bd.build_model(cfg)
    m.train()
    _check(m.backbone, True, frozen_stages=1, partial_bn=True)
    m.freeze_backbone()
    assert not any(p.requires_grad for p in m.backbone.parameters())
    m.unfreeze_backbone()
    assert all(p.requires_grad for p in m.backbone.parameters())
    m.train()
    _check(m.backbone, True, frozen_stages=1, partial_bn=True)
    assert m.backbone.conv1.bn.weight.requires_grad is False and m.backbone.layer2[0].conv1.conv.weight.requires_grad
    # The optimizer constructor groups as the reference's does (libs/models/cil_heads/tsm.py): frozen BatchNorm tensors are left
    # out, frozen conv weights stay listed and are skipped by the step for want of a gradient.  Every trainable tensor is held.
    opt = bd.build_optimizer(m, dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised',
                                     paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01, momentum=0.9, weight_decay=1e-4))
    held = {id(p) for g in opt.param_groups for p in g['params']}
    for name, p in m.named_parameters():
        if p.requires_grad:
            assert id(p) in held, name
        elif 'bn' in name.split('.'):
            assert id(p) not in held, name


@pytest.mark.parametrize('opts', [dict(), dict(norm_eval=True), dict(frozen_stages=0), dict(frozen_stages=2),
                                  dict(frozen_stages=1, norm_eval=True)],
                         ids=lambda o: ','.join(f'{k}={v}' for k, v in o.items()) or 'default')
def test_i3d_flags_after_train_eval_and_unfreeze(opts):
    m = ResNet3d(50, **opts)
    m.train()
    _check(m, True, **opts)
    m.eval()
    assert not any(b.training for _, b in _bns(m))
    for p in m.parameters():
        p.requires_grad = True
    m.train()
    _check(m, True, **opts)
    # the stem ConvModule as a whole goes to eval with the frozen stages (UPSTREAM ResNet3d._freeze_stages)
    assert m.conv1.training == (opts.get('frozen_stages', -1) < 0)


def test_options_are_named_constructor_parameters():
    sig = inspect.signature(ResNetTSM.__init__).parameters
    assert sig['frozen_stages'].default == -1 and sig['partial_bn'].default is False and sig['norm_eval'].default is False
    sig3 = inspect.signature(ResNet3d.__init__).parameters
    assert sig3['frozen_stages'].default == -1 and sig3['norm_eval'].default is False and 'partial_bn' not in sig3
    with pytest.raises(ValueError):
        ResNetTSM(18, frozen_stages=5)
    # the config dict is the interface
    m = bd.build_backbone(dict(type='ResNetTSM', depth=18, norm_eval=True, frozen_stages=1, partial_bn=True))
    assert (m.norm_eval, m.frozen_stages, m.partial_bn) == (True, 1, True)


def test_a_block_with_mixed_batchnorm_modes_is_named():
    m = ResNetTSM(18)
    m.train()
    m.layer2[0].conv2.bn.eval()
    with pytest.raises(ValueError, match=r'layer2\.0.*conv2\.bn: eval'):
        m.layer2[0].bn_training()
    assert m.layer2[1].bn_training() is True
    m.layer2[0].eval()
    assert m.layer2[0].bn_training() is False


def _header_params(hdr, name):
    m = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\((.*?)\);', hdr, re.S | re.M)
    assert m, f'{name} is not declared in include/bdvcil_hip.h'
    return [p.strip() for p in m.group(1).split(',')]


def test_entry_point_in_header_binding_and_library():
    raw = open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read()
    before = raw[:raw.index('int bdv_bn_eval_backward(')].rstrip()
    assert before.endswith('*/') and 'UPSTREAM' in before[before.rindex('/*'):], 'the declaration names the reference call site it stands for'
    hdr = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    params = _header_params(hdr, 'bdv_bn_eval_backward')
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    assert hasattr(lib, 'bdv_bn_eval_backward')
    res, args = bd._lib.SIGNATURES['bdv_bn_eval_backward']
    assert res is ctypes.c_int and len(args) == len(params), (len(args), params)
    for p, a in zip(params, args):
        assert ('*' in p) == (a is bd._lib.P), (p, a)
    assert bd._lib.lib().bdv_abi_version() == bd._lib.ABI_VERSION == 33
    assert callable(bd.kernels.bn_eval_backward)


def test_bad_arguments_fail_before_any_launch():
    """Argument errors need no GPU: the call returns before it launches (pointers are never dereferenced)."""
    lib = bd._lib.lib()
    one = ctypes.c_void_p(4096)

    def call(C=64, M=8, dy=one, mask=None, act=None, dz=None, dgamma=None, y=None, act_dtype=0):
        return lib.bdv_bn_eval_backward(ctypes.c_void_p(8192), mask, act, y, one, None, None, dy, dz, dgamma, None, 0.0, M, C, None, 0,
                                        act_dtype, 0, None, 0, None)
    assert call(C=96) == -1 and b'unsupported' in lib.bdv_last_error()
    assert call(C=80, mask=one) == -1
    assert call(dy=None) == -1 and b'null' in lib.bdv_last_error()
    assert call(M=0) == -1
    assert call(mask=one, act=one) == -1 and b'one ReLU sign source' in lib.bdv_last_error()
    assert call(dz=one) == -1 and b'distinct' in lib.bdv_last_error()          # dz aliases dy
    assert call(dgamma=one) == -1 and b'need y' in lib.bdv_last_error()        # parameter gradients without y / statistics
    assert call(act_dtype=7) == -1 and b'act_dtype' in lib.bdv_last_error()
    assert call(dy=ctypes.c_void_p(4100)) == -1 and b'alignment' in lib.bdv_last_error()
