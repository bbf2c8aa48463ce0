"""Host side of train_cfg.blending (no device needed): the reference's two blending configs build, the draws of MixupBlending /
CutmixBlending follow the restatement of UPSTREAM mmaction/datasets/blending_utils.py (parity unpinned: mmaction2 is not vendored,
the restatement is from memory of 0.24.x), the losses route soft labels by shape, and the C ABI declares the blend entry points."""
import copy
import ctypes
import json
import os

import pytest
import torch
from torch.distributions.beta import Beta

import bdvcil_amd as bd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'blending_configs.json')))


def ref_mixup_draw(B, alpha):
    """UPSTREAM MixupBlending.do_blending: Beta sample, then randperm."""
    lam = Beta(alpha, alpha).sample()
    perm = torch.randperm(B)
    return perm, lam


def ref_cutmix_draw(B, H, W, alpha):
    """UPSTREAM CutmixBlending.do_blending + rand_bbox: randperm, Beta sample, two randint; -> perm, (x1, y1, x2, y2), lam."""
    perm = torch.randperm(B)
    lam = Beta(alpha, alpha).sample()
    cut_rat = torch.sqrt(1. - lam)
    cut_w, cut_h = torch.tensor(int(W * cut_rat)), torch.tensor(int(H * cut_rat))
    cx = torch.randint(W, (1,))[0]
    cy = torch.randint(H, (1,))[0]
    x1, y1 = torch.clamp(cx - cut_w // 2, 0, W), torch.clamp(cy - cut_h // 2, 0, H)
    x2, y2 = torch.clamp(cx + cut_w // 2, 0, W), torch.clamp(cy + cut_h // 2, 0, H)
    lam = 1 - (1.0 * (x2 - x1) * (y2 - y1) / (W * H))
    return perm, (int(x1), int(y1), int(x2), int(y2)), lam


@pytest.mark.parametrize('rel,cls', [('recognition/tsm/tsm_r50_mixup_1x1x8_50e_sthv1_rgb.py', 'MixupBlending'),
                                     ('recognition/tsm/tsm_r50_cutmix_1x1x8_50e_sthv1_rgb.py', 'CutmixBlending')])
def test_reference_blending_configs_build(rel, cls):
    cfg = copy.deepcopy(CONFIGS[rel]['model'])
    assert cfg['type'] == 'Recognizer2D' and cfg['cls_head']['type'] == 'TSMHead' and cfg['train_cfg']['blending']['type'] == cls
    cfg['backbone']['pretrained'] = None
    m = bd.build_model(cfg)
    assert type(m) is bd.Recognizer2D and type(m.cls_head) is bd.TSMHead
    assert type(m.blending) is getattr(bd, cls) and type(m.blending).__name__ == cls
    assert m.blending.alpha == 0.2 and m.blending.num_classes == 174
    sd = m.cls_head.state_dict()
    assert list(sd) == ['fc_cls.weight', 'fc_cls.bias'] and sd['fc_cls.weight'].shape == (174, 2048)
    assert not hasattr(m.cls_head, 'inc_head_config')
    assert torch.count_nonzero(sd['fc_cls.bias']) == 0 and 0 < sd['fc_cls.weight'].std().item() < 2e-3      # N(0, init_std = 0.001)
    with pytest.raises(ValueError):
        m.cls_head.update_fc(180)


def test_no_train_cfg_no_blending():
    from oracle import tsm_oracle as O
    m = bd.build_model(O.r50_cfg(num_classes=7, depth=18))
    assert m.blending is None
    cfg = O.r50_cfg(num_classes=7, depth=18)
    cfg['train_cfg'] = dict(aux_info=[])                      # a train_cfg without the key
    assert bd.build_model(cfg).blending is None
    cfg['train_cfg'] = dict(blending=dict(type='MixupBlending', num_classes=7, alpha=1.0))
    assert isinstance(bd.build_model(cfg).blending, bd.MixupBlending)
    i3d = dict(type='Recognizer3D',
               backbone=dict(type='ResNet3d', pretrained2d=True, pretrained=None, depth=50, conv1_kernel=(5, 7, 7), conv1_stride_t=2,
                             pool1_stride_t=2, conv_cfg=dict(type='Conv3d'), norm_eval=False,
                             inflate=((1, 1, 1), (1, 0, 1, 0), (1, 0, 1, 0, 1, 0), (0, 1, 0)), zero_init_residual=False),
               cls_head=dict(type='I3DHead', num_classes=5, in_channels=2048, spatial_type='avg', dropout_ratio=0.0, init_std=0.01),
               train_cfg=None, test_cfg=dict(average_clips='prob'))
    assert bd.build_model(copy.deepcopy(i3d)).blending is None
    i3d['train_cfg'] = dict(blending=dict(type='CutmixBlending', num_classes=5, alpha=.2))
    assert isinstance(bd.build_model(i3d).blending, bd.CutmixBlending)


def test_build_blending_registry():
    assert 'MixupBlending' in bd.BLENDINGS and 'CutmixBlending' in bd.BLENDINGS and 'Recognizer2D' in bd.RECOGNIZERS and 'TSMHead' in bd.HEADS
    with pytest.raises(KeyError):
        bd.build_blending(dict(type='Nope'))
    b = bd.build_blending(dict(type='CutmixBlending', num_classes=3))
    assert b.alpha == .2 and b.num_classes == 3


@pytest.mark.parametrize('seed', range(8))
def test_draws_follow_the_restatement(seed):
    B, H, W = 4, 20, 28
    for alpha in (1.0, 0.2):
        torch.manual_seed(seed)
        perm, lam = ref_mixup_draw(B, alpha)
        after = torch.rand(1)
        torch.manual_seed(seed)
        p, box, l = bd.MixupBlending(9, alpha).draw(B, H, W)
        assert torch.equal(p, perm) and box is None and l == float(lam) and torch.equal(torch.rand(1), after)
        torch.manual_seed(seed)
        perm, (x1, y1, x2, y2), lam = ref_cutmix_draw(B, H, W, alpha)
        after = torch.rand(1)
        torch.manual_seed(seed)
        p, box, l = bd.CutmixBlending(9, alpha).draw(B, H, W)
        assert torch.equal(p, perm) and box == (y1, x1, y2, x2) and l == float(lam) and torch.equal(torch.rand(1), after)
        assert lam.dtype == torch.float32 and 0 <= box[0] <= box[2] <= H and 0 <= box[1] <= box[3] <= W


def test_losses_route_soft_labels_by_shape(monkeypatch):
    L = bd.losses
    calls = []
    monkeypatch.setattr(L, '_soft_label_ce', lambda s, t, cw: calls.append('soft') or s.sum())
    monkeypatch.setattr(L, '_weighted_ce', lambda s, t, cw: calls.append('hard') or s.sum())
    ce = bd.CrossEntropyLoss()
    score = torch.zeros(4, 9)
    ce(score, torch.zeros(4, 9))
    ce(score, torch.zeros(4, dtype=torch.int64))
    ce(torch.zeros(1, 9), torch.tensor(3))                                 # a 0-dim label of a batch of one
    ce(score, torch.zeros(4, 9), num_classes=9, batch_data={})              # the kwargs CILRecognizer2D adds
    assert calls == ['soft', 'hard', 'hard', 'soft']
    assert L.is_soft_label(score, torch.zeros(4, 9)) and not L.is_soft_label(score, torch.zeros(4, 1)) \
        and not L.is_soft_label(score, torch.zeros(9, 4)) and not L.is_soft_label(score, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='CrossEntropyLoss'):
        bd.LSCLoss()(score, torch.zeros(4, 9))
    from bdvcil_amd.recognizer import hard_labels
    soft1 = torch.zeros(1, 9)
    assert hard_labels(soft1) is soft1 and hard_labels(torch.zeros(4, 1, dtype=torch.int64)).shape == (4,)


def test_blend_symbols_are_declared():
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read()
    for name, nargs in (('bdv_blend_mix_f32', 7), ('bdv_blend_box_scratch_bytes', 7), ('bdv_blend_box_f32', 14)):
        assert name in bd._lib.SIGNATURES and len(bd._lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name) and name + '(' in hdr
    assert bd._lib.SIGNATURES['bdv_blend_box_scratch_bytes'][0] is ctypes.c_size_t
    assert 'blend.hip' in bd._lib.HASHED_SOURCES
    sb = bd._lib.lib().bdv_blend_box_scratch_bytes
    assert sb(4, 6, 1, 0, 0, 0, 0) == 0 and sb(4, 6, 1, 2, 1, 2, 6) == 0                # empty boxes
    assert sb(4, 6, 1, 2, 3, 3, 4) == 4 * 6 * 1 * 16                                    # one pixel: one 16-byte unit per row
    assert sb(4, 6, 1, 0, 0, 5, 7) >= 4 * 6 * 5 * 7 * 4 and sb(4, 2, 4, 0, 0, 5, 7) >= 4 * 2 * 5 * 7 * 16


def test_wrappers_refuse_before_touching_the_device():
    K = bd.kernels
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.blend_mix(torch.zeros(4, 6), torch.arange(4), 0.5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.blend_box_(torch.zeros(4, 6, 5, 7), torch.arange(4), (0, 0, 1, 1), 6, 5, 7)
    with pytest.raises(ValueError):
        K._blend_perm(torch.tensor([0, 1, 2, 4]), 4, 'cpu', 't')
    with pytest.raises(ValueError):
        K._blend_perm(torch.tensor([0, -1, 2, 3]), 4, 'cpu', 't')
    with pytest.raises(ValueError):
        K._blend_perm(torch.arange(3), 4, 'cpu', 't')
