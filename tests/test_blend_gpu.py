"""The clip-blend kernels (csrc/blend.hip), MixupBlending / CutmixBlending and the recognizers' train_cfg.blending against torch on the
CPU: pixels bit for bit, labels within two fp32 roundings, losses within the step tests' relative bound.

The CPU restatement of UPSTREAM mmaction/datasets/blending_utils.py below is from memory of mmaction2 0.24.x (parity unpinned: it is
not vendored by the reference).  The index vectors of the kernel tests have four entries; on the shapes with three samples their
three-entry counterparts are used ([1, 2, 0] for the cycles, [0, 2, 1] for a fixed point beside a swap), and on the 4 x 4 grid the boxes
are clipped to it."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions.beta import Beta

from oracle import tsm_oracle as O

pytestmark = pytest.mark.gpu

LABEL_TOL = 2.0 ** -22          # two fp32 roundings of values in [0, 1]


def _x(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- kernels ------------------------------------------------------------------------------------------------------------------

MIX_SHAPES = [(4, 2, 3, 5, 7), (3, 1, 3, 4, 4), (8, 5, 7, 4)]      # the last: Nhwc4 frames of B = 4, T = 2
MIX_PERMS = {4: [[0, 1, 2, 3], [1, 2, 0, 3], [3, 2, 1, 0]], 3: [[0, 1, 2], [1, 2, 0], [2, 1, 0]]}
LAMS = [0.0, 1.0, 0.3, 0.655668]


@pytest.mark.parametrize('shape', MIX_SHAPES)
def test_blend_mix_is_torchs_expression_bit_for_bit(shape, dev):
    from bdvcil_amd import kernels as K
    B = 3 if shape[0] == 3 else 4
    x = _x(shape)
    xs = x.view(B, -1)                                      # samples first (the Nhwc4 tensor has B * T rows)
    xg = xs.to(dev)
    for perm in MIX_PERMS[B]:
        for lam in LAMS:
            lam_t = torch.tensor(lam, dtype=torch.float32)  # 0-dim fp32, as Beta.sample() returns
            want = lam_t * xs + (1 - lam_t) * xs[torch.tensor(perm)]
            got = K.blend_mix(xg, torch.tensor(perm), lam_t)
            assert got.data_ptr() != xg.data_ptr() and torch.equal(got.cpu(), want), (perm, lam)
            assert torch.equal(K.blend_mix(xg, perm, float(lam_t)).cpu(), want)         # a list and a Python float do as well
    assert torch.equal(xg.cpu(), xs)                        # the input is left alone


BOXES = [(0, 0, 5, 7), (2, 3, 3, 4), (0, 0, 0, 0), (2, 1, 2, 6), (0, 1, 5, 6), (4, 0, 5, 7), (1, 5, 4, 7)]
BOX_PERMS = {4: [[1, 3, 2, 0], [2, 3, 1, 0], [0, 1, 2, 3], [0, 0, 0, 0]], 3: [[1, 2, 0], [0, 2, 1], [0, 1, 2], [0, 0, 0]]}
# shape, B, outer, H, W, inner
BOX_SHAPES = [((4, 2, 3, 5, 7), 4, 6, 5, 7, 1), ((3, 1, 3, 4, 4), 3, 3, 4, 4, 1), ((8, 5, 7, 4), 4, 2, 5, 7, 4), ((3, 2, 3, 2, 5, 7), 3, 12, 5, 7, 1)]


@pytest.mark.parametrize('shape,B,outer,H,W,inner', BOX_SHAPES)
def test_blend_box_is_gather_then_assign(shape, B, outer, H, W, inner, dev):
    from bdvcil_amd import kernels as K
    x = _x(shape, seed=1)
    v = x.view(B, outer, H, W, inner)
    for perm in BOX_PERMS[B]:
        for box in BOXES:
            r1, c1, r2, c2 = min(box[0], H), min(box[1], W), min(box[2], H), min(box[3], W)
            want = v.clone()
            want[:, :, r1:r2, c1:c2, :] = want[torch.tensor(perm)][:, :, r1:r2, c1:c2, :]
            xg = x.clone().to(dev)
            ret = K.blend_box_(xg, torch.tensor(perm), (r1, c1, r2, c2), outer, H, W, inner)
            assert ret is xg
            got = xg.cpu().view(B, outer, H, W, inner)
            assert torch.equal(got, want), (perm, box)
            outside = torch.ones(H, W, dtype=torch.bool)
            outside[r1:r2, c1:c2] = False
            assert torch.equal(got[:, :, outside, :], v[:, :, outside, :]), (perm, box)
            if r1 == r2 or c1 == c2:
                assert torch.equal(got, v)


def test_blend_refusals(dev):
    from bdvcil_amd import _lib
    from bdvcil_amd import kernels as K
    x = _x((4, 2, 3, 5, 7), seed=2)
    xg = x.to(dev)
    perm = torch.tensor([1, 2, 0, 3])
    with pytest.raises(_lib.HipExtensionError, match='alias'):
        K.blend_mix(xg, perm, 0.5, out=xg)
    with pytest.raises(_lib.HipExtensionError, match='alias'):
        K.blend_mix(xg.view(-1)[:630].view(3, 210), [1, 2, 0], 0.5, out=xg.view(-1)[210:].view(3, 210))    # a partial overlap
    for box in [(0, 0, 6, 7), (0, 0, 5, 8), (-1, 0, 5, 7), (3, 0, 2, 7), (0, 5, 5, 4)]:
        with pytest.raises(ValueError, match='outside'):
            K.blend_box_(xg, perm, box, 6, 5, 7)
    # the library refuses the same on its own (the wrapper's check is not the only one)
    ws = K.workspace(1 << 20, dev, 'blend')
    pd = perm.to(dev)
    code = _lib.lib().bdv_blend_box_f32(xg.data_ptr(), pd.data_ptr(), 4, 6, 5, 7, 1, 0, 0, 6, 7, ws.data_ptr(), ws.numel(), None)
    assert code != 0 and b'outside' in _lib.lib().bdv_last_error()
    assert _lib.lib().bdv_blend_box_f32(xg.data_ptr(), pd.data_ptr(), 4, 6, 5, 7, 2, 0, 0, 5, 7, ws.data_ptr(), ws.numel(), None) != 0    # inner 2
    assert _lib.lib().bdv_blend_box_f32(xg.data_ptr(), pd.data_ptr(), 4, 6, 5, 7, 1, 0, 0, 5, 7, ws.data_ptr(), 64, None) != 0           # scratch
    assert _lib.lib().bdv_blend_box_f32(xg.data_ptr(), pd.data_ptr(), 4, 6, 5, 7, 1, 0, 0, 5, 7, None, 0, None) != 0                     # null scratch
    with pytest.raises(ValueError, match='perm'):
        K.blend_mix(xg, [1, 2, 4, 3], 0.5)
    with pytest.raises(ValueError, match='perm'):
        K.blend_box_(xg, [1, 2, 4, 3], (0, 0, 5, 7), 6, 5, 7)
    with pytest.raises(ValueError):
        K.blend_box_(xg, perm, (0, 0, 5, 7), 6, 5, 7, inner=2)
    with pytest.raises(TypeError):
        K.blend_mix(xg.half(), perm, 0.5)
    with pytest.raises(TypeError):
        K.blend_box_(xg.half(), perm, (0, 0, 5, 7), 6, 5, 7)
    with pytest.raises(TypeError):
        K.blend_mix(xg, perm.to(dev), 0.5)                                  # the range check needs the host copy
    with pytest.raises(ValueError):
        K.blend_box_(xg.permute(0, 1, 2, 4, 3), perm, (0, 0, 5, 7), 6, 7, 5)       # not contiguous
    torch.cuda.synchronize()
    assert torch.equal(xg.cpu(), x)                                         # nothing was launched


# ---- the blending classes -----------------------------------------------------------------------------------------------------

def ref_mixup(imgs, label, num_classes, alpha):
    """UPSTREAM MixupBlending on CPU tensors: -> (new imgs, (B, K) labels, perm)."""
    onehot = F.one_hot(label.view(-1), num_classes)
    lam = Beta(alpha, alpha).sample()
    perm = torch.randperm(imgs.size(0))
    return lam * imgs + (1 - lam) * imgs[perm], lam * onehot + (1 - lam) * onehot[perm], perm


def ref_cutmix(imgs, label, num_classes, alpha):
    """UPSTREAM CutmixBlending on CPU tensors, ``imgs`` modified in place: -> (imgs, (B, K) labels, perm, box (x1, y1, x2, y2))."""
    onehot = F.one_hot(label.view(-1), num_classes)
    W, H = imgs.size(-1), imgs.size(-2)
    perm = torch.randperm(imgs.size(0))
    lam = Beta(alpha, alpha).sample()
    cut_rat = torch.sqrt(1. - lam)
    cut_w, cut_h = torch.tensor(int(W * cut_rat)), torch.tensor(int(H * cut_rat))
    cx = torch.randint(W, (1,))[0]
    cy = torch.randint(H, (1,))[0]
    x1, y1 = torch.clamp(cx - cut_w // 2, 0, W), torch.clamp(cy - cut_h // 2, 0, H)
    x2, y2 = torch.clamp(cx + cut_w // 2, 0, W), torch.clamp(cy + cut_h // 2, 0, H)
    imgs[..., y1:y2, x1:x2] = imgs[perm][..., y1:y2, x1:x2]
    lam = 1 - (1.0 * (x2 - x1) * (y2 - y1) / (W * H))
    return imgs, lam * onehot + (1 - lam) * onehot[perm], perm, (int(x1), int(y1), int(x2), int(y2))


def _check_labels(got, want, K_):
    got = got.cpu()
    assert got.shape == want.shape == (want.shape[0], K_) and got.dtype == torch.float32
    err = (got - want).abs().max().item()
    rows = (got.double().sum(1) - 1).abs().max().item()
    print(f'labels: max abs err {err:.3e}, rows sum to 1 within {rows:.3e} (bound {LABEL_TOL:.3e})')
    assert err <= LABEL_TOL and rows <= LABEL_TOL


def _nhwc4(x, dev):
    """(B, T, 3, H, W) CPU clips -> the front-end's Nhwc4Frames on the device."""
    import bdvcil_amd as bd
    B, T, _, H, W = x.shape
    return bd.Nhwc4Frames(bd.kernels.nchw3_to_nhwc4(x.reshape(B * T, 3, H, W).to(dev)), B, T)


def _from_nhwc4(fr):
    d = fr.data.cpu()
    assert torch.count_nonzero(d[..., 3]) == 0
    return d[..., :3].permute(0, 3, 1, 2).reshape(fr.batches, fr.num_segments, 3, d.shape[1], d.shape[2])


CLS_B, CLS_T, CLS_H, CLS_W, CLS_K = 4, 2, 20, 28, 9
MIXUP_PERMS = {3: [1, 2, 0, 3], 2: [0, 1, 2, 3]}
CUTMIX_PERMS = {1: [1, 3, 2, 0], 3: [2, 3, 1, 0]}


@pytest.mark.parametrize('seed', range(8))
def test_mixup_blending(seed, dev):
    import bdvcil_amd as bd
    x = _x((CLS_B, CLS_T, 3, CLS_H, CLS_W), seed=10)
    label = torch.randint(0, CLS_K, (CLS_B, 1), generator=torch.Generator().manual_seed(11))
    torch.manual_seed(seed)
    want, wlab, perm = ref_mixup(x.clone(), label, CLS_K, 1.0)
    if seed in MIXUP_PERMS:
        assert perm.tolist() == MIXUP_PERMS[seed]
    blend = bd.MixupBlending(CLS_K, alpha=1.0)
    torch.manual_seed(seed)
    xg = x.to(dev)
    got, lab = blend(xg, label.to(dev))
    assert got is not xg and torch.equal(xg.cpu(), x) and torch.equal(got.cpu(), want)
    _check_labels(lab, wlab, CLS_K)
    torch.manual_seed(seed)
    fr = _nhwc4(x, dev)
    got4, lab4 = blend(fr, label.view(-1).to(dev))                         # (B,) labels as well as (B, 1)
    assert isinstance(got4, bd.Nhwc4Frames) and got4 is not fr and got4.data.data_ptr() != fr.data.data_ptr()
    assert (got4.batches, got4.num_segments) == (CLS_B, CLS_T) and torch.equal(_from_nhwc4(got4), want) and torch.equal(_from_nhwc4(fr), x)
    assert torch.equal(lab4, lab)


@pytest.mark.parametrize('seed,alpha', [(s, 1.0) for s in range(8)] + [(1, 0.2)])
def test_cutmix_blending(seed, alpha, dev):
    import bdvcil_amd as bd
    x = _x((CLS_B, CLS_T, 3, CLS_H, CLS_W), seed=10)
    label = torch.randint(0, CLS_K, (CLS_B, 1), generator=torch.Generator().manual_seed(11))
    torch.manual_seed(seed)
    want, wlab, perm, (x1, y1, x2, y2) = ref_cutmix(x.clone(), label, CLS_K, alpha)
    assert x2 > x1 and y2 > y1                                               # a non-empty box on every case
    if alpha == 1.0 and seed in CUTMIX_PERMS:
        assert perm.tolist() == CUTMIX_PERMS[seed]
    blend = bd.CutmixBlending(CLS_K, alpha=alpha)
    torch.manual_seed(seed)
    xg = x.to(dev)
    got, lab = blend(xg, label.to(dev))
    assert got is xg and torch.equal(xg.cpu(), want)                        # in place, the same object
    _check_labels(lab, wlab, CLS_K)
    torch.manual_seed(seed)
    fr = _nhwc4(x, dev)
    got4, lab4 = blend(fr, label.to(dev))
    assert got4 is fr and torch.equal(_from_nhwc4(fr), want) and torch.equal(lab4, lab)


# ---- the recognizers ----------------------------------------------------------------------------------------------------------

def _pair(K_, dev, blending=None, seed=0):
    """The needed lines of test_model_gpu._pair: an R18 / SimpleLinear / CrossEntropyLoss oracle and HIP model with the same weights
    and perturbed BatchNorm parameters; ``blending`` goes into the HIP model's train_cfg only."""
    import bdvcil_amd as bd
    torch.manual_seed(seed)
    cfg = O.r50_cfg(num_classes=K_, depth=18, head='SimpleLinear', loss='CrossEntropyLoss', dropout_ratio=0.0)
    ref = O.build_model(copy.deepcopy(cfg))
    g = torch.Generator().manual_seed(seed + 1)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5, generator=g)
            m.bias.data.normal_(0, 0.1, generator=g)
            m.running_mean.normal_(0, 0.1, generator=g)
            m.running_var.uniform_(0.5, 1.5, generator=g)
    cfg = copy.deepcopy(cfg)
    if blending is not None:
        cfg['train_cfg'] = dict(blending=blending)
    mod = bd.build_model(cfg)
    mod.load_state_dict(ref.state_dict())
    return ref, mod.to(dev)


@pytest.mark.parametrize('kind', ['MixupBlending', 'CutmixBlending'])
def test_recognizer2d_trains_on_blended_clips(kind, dev):
    K_ = 9
    ref, mod = _pair(K_, dev, blending=dict(type=kind, num_classes=K_, alpha=1.0))
    _, plain = _pair(K_, dev)
    assert type(mod.blending).__name__ == kind and plain.blending is None
    for m in (ref, mod, plain):
        m.test_cfg['average_clips'] = 'score'
    g = torch.Generator().manual_seed(100)
    imgs, labels = torch.randn(4, 8, 3, 64, 64, generator=g), torch.randint(0, K_, (4, 1), generator=g)
    # blending is off at test time: the logits are those of a model built without train_cfg, and the clips are left alone
    mod.eval(); plain.eval()
    xg = imgs.to(dev)
    with torch.no_grad():
        assert torch.equal(mod(xg, return_loss=False), plain(xg, return_loss=False))
    assert torch.equal(xg.cpu(), imgs)
    ref.train(); mod.train()
    torch.manual_seed(5)
    if kind == 'MixupBlending':
        x_mixed, label_mixed, perm = ref_mixup(imgs.clone(), labels, K_, 1.0)
    else:
        x_mixed, label_mixed, perm, _ = ref_cutmix(imgs.clone(), labels, K_, 1.0)
    assert perm.tolist() != [0, 1, 2, 3] and not torch.equal(x_mixed, imgs)
    with torch.no_grad():
        rloss = O.soft_target_ce(ref(x_mixed, return_loss=False), label_mixed.float()).item()
        unmixed = F.cross_entropy(ref(imgs, return_loss=False), labels.view(-1)).item()
    torch.manual_seed(5)
    out = mod(xg, labels.to(dev))
    loss = out['loss_cls']
    print(f'{kind}: loss {loss.item():.6f}, oracle on the mixed clips {rloss:.6f}, oracle without blending {unmixed:.6f}')
    assert abs(loss.item() - rloss) <= 1e-4 * max(1.0, abs(rloss))
    assert abs(unmixed - rloss) > 1e-3 * max(1.0, abs(rloss))               # the case tells a model that skips the blending apart
    assert 'top1_acc' not in out and 'top5_acc' not in out
    assert torch.equal(xg.cpu(), x_mixed if kind == 'CutmixBlending' else imgs)     # CutMix works in place, Mixup does not
    loss.backward()
    grads = [p.grad for p in mod.parameters() if p.requires_grad]
    assert all(gr is not None for gr in grads)
    assert bool(torch.stack([torch.isfinite(gr).all() for gr in grads]).all())
    assert any(float(gr.abs().max()) > 0 for gr in grads[:3])


def test_recognizer3d_blends_before_forward_train(dev):
    """Recognizer3D with a Mixup blending == the same model without one, fed the hand-mixed clips and soft labels."""
    import bdvcil_amd as bd
    K_ = 5
    cfg = dict(type='Recognizer3D',
               backbone=dict(type='ResNet3d', pretrained2d=True, pretrained=None, depth=50, conv1_kernel=(5, 7, 7), conv1_stride_t=2,
                             pool1_stride_t=2, conv_cfg=dict(type='Conv3d'), norm_eval=False,
                             inflate=((1, 1, 1), (1, 0, 1, 0), (1, 0, 1, 0, 1, 0), (0, 1, 0)), zero_init_residual=False),
               cls_head=dict(type='I3DHead', num_classes=K_, in_channels=2048, spatial_type='avg', dropout_ratio=0.0, init_std=0.01),
               train_cfg=None, test_cfg=dict(average_clips='prob'))
    torch.manual_seed(0)
    plain = bd.build_model(copy.deepcopy(cfg))
    cfg['train_cfg'] = dict(blending=dict(type='MixupBlending', num_classes=K_, alpha=1.0))
    mod = bd.build_model(cfg)
    mod.load_state_dict(plain.state_dict())
    plain.to(dev).train(); mod.to(dev).train()
    g = torch.Generator().manual_seed(7)
    imgs, labels = torch.randn(4, 1, 3, 8, 64, 64, generator=g), torch.randint(0, K_, (4, 1), generator=g)
    torch.manual_seed(3)
    x_mixed, label_mixed, perm = ref_mixup(imgs.clone(), labels, K_, 1.0)
    assert perm.tolist() == [1, 2, 0, 3]
    xg = imgs.to(dev)
    torch.manual_seed(3)
    hand_x, hand_label = mod.blending(xg, labels.to(dev))                   # mixed by hand: the same draws, outside the model
    assert torch.equal(hand_x.cpu(), x_mixed)
    _check_labels(hand_label, label_mixed.float(), K_)
    with torch.no_grad():
        want = plain(hand_x, hand_label)
        torch.manual_seed(3)
        got = mod(xg, labels.to(dev))
    assert 'top1_acc' not in got and 'top1_acc' not in want
    assert torch.equal(got['loss_cls'], want['loss_cls'])
    assert torch.equal(xg.cpu(), imgs)


def test_video_mix_step_takes_nhwc4_frames(dev):
    """icarl_video_mix_training_step on the front-end's Nhwc4Frames: the loss and the mixed clips of the (B, T, 3, H, W) path."""
    import bdvcil_amd as bd
    K_, prevK = 9, 4
    _, mod = _pair(K_, dev)
    _, prev = _pair(K_, dev, seed=9)
    mod.test_cfg['average_clips'] = prev.test_cfg['average_clips'] = 'score'
    mod.train(); prev.eval()
    g = torch.Generator().manual_seed(100)
    imgs, labels = torch.randn(4, 8, 3, 64, 64, generator=g), torch.randint(0, K_, (4, 1), generator=g)
    labels[0, 0], labels[3, 0] = 2, 7
    mixed = 0
    for seed in range(4):
        def seeds():
            random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
        seeds()
        x5 = imgs.to(dev)
        with torch.no_grad():
            l5 = bd.icarl_video_mix_training_step(mod, dict(imgs=x5, label=labels.to(dev)), K_, 0.6, 0.8, current_task=1, prev_model=prev,
                                                  previous_task_num_classes=prevK)
        seeds()
        fr = _nhwc4(imgs, dev)
        with torch.no_grad():
            l4 = bd.icarl_video_mix_training_step(mod, dict(imgs=fr, label=labels.to(dev)), K_, 0.6, 0.8, current_task=1, prev_model=prev,
                                                  previous_task_num_classes=prevK)
        assert torch.equal(l4, l5), seed
        assert torch.equal(_from_nhwc4(fr), x5.cpu())
        mixed += int(not torch.equal(x5.cpu(), imgs))
    assert 0 < mixed < 4
