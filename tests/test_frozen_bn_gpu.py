"""Training steps through eval-mode BatchNorm -- ``norm_eval``, ``partial_bn``, ``frozen_stages`` -- against the CPU oracle.

The comparison is ``tests/test_model_gpu.py::test_train_step``'s: gradients are judged against the fp64 run of the oracle, the ReLU
sign bits of the HIP path are read back through the taps, and a parameter is held to  relL2 <= 3 * e_f32 + 1e-4  when no flipped
sign lies behind it and to  3 * e_f32 + 1e-2  when one does (e_f32: the fp32 CPU oracle's own error against fp64); every flip
must sit within 1e-5 of its channel's scale of zero in fp64.  The oracle knows ``norm_eval``; ``frozen_stages`` and ``partial_bn``
are set on its modules by name (the module trees agree)."""
import copy

import pytest
import torch

from oracle import tsm_oracle as O
from test_model_gpu import (ReluRecorder, _clips, _oracle_only, _rel, _rel_l2, _report, count_pool_flips, count_relu_flips,
                            relu_site_owners)

pytestmark = pytest.mark.gpu

K_ = 11
MODES = {
    'norm_eval': dict(norm_eval=True),
    'partial_bn': dict(partial_bn=True),
    'frozen1': dict(frozen_stages=1, norm_eval=False),
    'frozen1_norm_eval': dict(frozen_stages=1, norm_eval=True),
}
OPT_CFG = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0),
               lr=0.01, momentum=0.9, weight_decay=1e-4)


def _set_oracle_mode(ref, norm_eval=False, partial_bn=False, frozen_stages=-1):
    """UPSTREAM ResNet.train(True) with the three options, on the oracle's modules."""
    ref.train()
    bb = ref.backbone
    if frozen_stages >= 0:
        bb.conv1.bn.eval()
        for p in bb.conv1.parameters():
            p.requires_grad = False
    for i in range(1, frozen_stages + 1):
        layer = getattr(bb, f'layer{i}')
        layer.eval()
        for p in layer.parameters():
            p.requires_grad = False
    bns = [m for m in bb.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    if norm_eval:
        for m in bns:
            m.eval()
    if partial_bn:
        for m in bns[1:]:
            m.eval()
            m.weight.requires_grad = False
            m.bias.requires_grad = False


def _hip_model(ref, cfg, opts, dev):
    import bdvcil_amd as bd
    cfg = copy.deepcopy(cfg)
    cfg['backbone'].update(opts)
    mod = bd.build_model(cfg)
    mod.load_state_dict(ref.state_dict())
    return mod.to(dev)


_ORACLE = {}


def _oracle_step(depth, mode, opts, freeze=None):
    """fp32 and fp64 CPU steps of one (depth, mode): run once, shared by the conv arithmetics, never modified afterwards.
    ``freeze``: applied to each oracle's backbone after the mode is set."""
    key = (depth, mode)
    if key not in _ORACLE:
        ref, cfg = _oracle_only(depth, 'SimpleLinear', 'CrossEntropyLoss', K=K_, want_cfg=True)
        state = copy.deepcopy(ref.state_dict())
        ref64 = copy.deepcopy(ref).double()
        imgs, labels = _clips(2, 8, 64, K_, seed=5)
        for m in (ref, ref64):
            _set_oracle_mode(m, **opts)
            if freeze is not None:
                freeze(m.backbone)
        with ReluRecorder() as rec32:
            rl = ref(imgs, labels)
        rl['loss_cls'].backward()
        with ReluRecorder() as rec:
            r64 = ref64(imgs.double(), labels)
        r64['loss_cls'].backward()
        _ORACLE[key] = dict(ref=ref, ref64=ref64, cfg=cfg, state=state, imgs=imgs, labels=labels, loss=rl['loss_cls'].item(),
                            pre32=rec32.pre, pre64=rec.pre)
    return _ORACLE[key]


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('depth', [18, 50])
def test_train_step_through_eval_batchnorm(depth, mode, dev, conv_arith):
    _check_train_step(depth, mode, MODES[mode], dev, conv_arith)


def _check_train_step(depth, mode, opts, dev, conv_arith, freeze=None):
    """One training step of the HIP model under the backbone options ``opts`` against the oracle's, by the rule in this file's
    docstring.  ``freeze``: applied to every backbone (both oracles, the model) after ``train()``.  Returns (model, oracle step)."""
    from bdvcil_amd import functional as Fn
    o = _oracle_step(depth, mode, opts, freeze)
    ref, ref64 = o['ref'], o['ref64']
    mod = _hip_model(_StateOnly(o['state']), o['cfg'], opts, dev)
    mod.train()
    if freeze is not None:
        freeze(mod.backbone)
    eval_bns = {n for n, m in mod.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and not m.training}
    ref_eval = {n for n, m in ref.named_modules() if isinstance(m, torch.nn.BatchNorm2d) and not m.training}
    assert eval_bns == ref_eval and eval_bns
    buffers_before = {n: b.detach().clone() for n, b in mod.named_buffers()}
    Fn.RELU_MASK_TAP = taps = []
    Fn.POOL_IDX_TAP = pool_idx = []
    try:
        ol = mod(o['imgs'].to(dev), o['labels'].to(dev), batch_data=None)
    finally:
        Fn.RELU_MASK_TAP = Fn.POOL_IDX_TAP = None
    ol['loss_cls'].backward()
    torch.cuda.synchronize()
    assert abs(ol['loss_cls'].item() - o['loss']) <= 1e-4 * max(1.0, abs(o['loss']))

    # ReLU signs: the sites of frozen stages run without a backward pass and write no bits; every other site does
    owners = relu_site_owners(ref)
    frozen = opts.get('frozen_stages', -1)
    n_frozen = 0 if frozen < 0 else 1 + sum(len(getattr(ref.backbone, f'layer{i}')) * (2 if depth == 18 else 3) for i in range(1, frozen + 1))
    assert len(taps) == len(owners) - n_frozen
    flips, flips32 = count_relu_flips(o['pre64'][n_frozen:], o['pre32'][n_frozen:], taps)
    last_flip = max([k + n_frozen for k, n in enumerate(flips) if n], default=-1)
    pool_flips = 0
    if frozen < 0:
        pool_flips = count_pool_flips(o['pre64'][0], o['pre32'][0], pool_idx[0])
        if pool_flips:
            last_flip = max(last_flip, 0)
    _report(f'[eval-BN relu flips] R{depth} {mode} {conv_arith}: {sum(flips)} signs differ from the fp64 oracle at sites '
            f'{[k + n_frozen for k, n in enumerate(flips) if n]} (fp32 CPU oracle: {sum(flips32)}); stem arg-max differs at {pool_flips}')

    def behind_a_flip(name):
        for k, prefixes in enumerate(owners):
            if any(name.startswith(q) for q in prefixes):
                return k <= last_flip
        return False
    rp, r64p, op = dict(ref.named_parameters()), dict(ref64.named_parameters()), dict(mod.named_parameters())
    worst, n_frozen_params = {}, 0
    for name, p in rp.items():
        assert op[name].requires_grad == p.requires_grad, name
        if not p.requires_grad:                 # frozen by the mode: no gradient at all
            assert p.grad is None and op[name].grad is None, name
            n_frozen_params += 1
            continue
        assert p.grad is not None and op[name].grad is not None, name
        e_hip = _rel_l2(op[name].grad, r64p[name].grad)
        e_f32 = _rel_l2(p.grad, r64p[name].grad)
        loose = behind_a_flip(name)
        print(f'{name}: relL2 hip {e_hip:.3e}, fp32 CPU {e_f32:.3e}, {"behind a flip" if loose else "no flip behind"}')
        assert e_hip <= 3 * e_f32 + (1e-2 if loose else 1e-4), (name, e_hip, e_f32, 'behind a flipped ReLU' if loose else 'no flip behind it', flips)
        if e_hip > worst.get(loose, (0,))[0]:
            worst[loose] = (e_hip, e_f32, name)
    assert (n_frozen_params > 0) == (mode != 'norm_eval')
    _report(f'[eval-BN grad parity] R{depth} {mode} {conv_arith}: worst (relL2 hip, relL2 fp32 CPU, name) with no flip behind: '
            f'{worst.get(False)}; behind a flip: {worst.get(True)}')

    # running statistics: untouched bit for bit where the BatchNorm ran in eval mode, the oracle's where it ran in train mode
    rb, ob = dict(ref.named_buffers()), dict(mod.named_buffers())
    for name, b in rb.items():
        owner = name.rsplit('.', 1)[0]
        if owner in eval_bns:
            assert torch.equal(ob[name], buffers_before[name]), name
        elif name.endswith('num_batches_tracked'):
            assert int(ob[name].item()) == int(b.item()) == 1, name
        else:
            assert _rel(ob[name], b) <= 1e-4, name
    return mod, o


def _freeze_mixed(backbone):
    """Live and frozen BatchNorm affines side by side inside the blocks of a TSM-R50.  Units (conv1, conv2, conv3) by block:
    layer1 / layer2 / layer4 live-live-live in the even blocks and live-frozen-live in the odd ones, layer3 frozen-live-live and
    frozen-frozen-live; conv3 frozen in layer2.0 and layer4.0, the downsample in layer3.0 and layer4.0, so that the four
    downsample blocks cover the four (last unit, downsample) combinations.  Every block without a downsample branch ends in a
    live unit: the all-frozen ending without one is ``partial_bn``'s."""
    frozen = []
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(backbone, f'layer{li}')):
            frozen += [blk.conv2.bn] if bi % 2 else []
            frozen += [blk.conv1.bn] if li == 3 else []
            frozen += [blk.conv3.bn] if bi == 0 and li in (2, 4) else []
            frozen += [blk.downsample.bn] if bi == 0 and li in (3, 4) else []
    for bn in frozen:
        bn.weight.requires_grad = False
        bn.bias.requires_grad = False


def test_train_step_with_mixed_affine_units(dev, conv_arith):
    """``norm_eval`` with some BatchNorm affines frozen inside a block (``_freeze_mixed``): the gradient rule, ``grad is None``
    for the frozen tensors and the untouched buffers of ``test_train_step_through_eval_batchnorm``; then the stage nodes and
    the block nodes give the same bits."""
    from bdvcil_amd import functional as Fn
    mod, o = _check_train_step(50, 'mixed', dict(norm_eval=True), dev, conv_arith, freeze=_freeze_mixed)
    bb = mod.backbone
    live = lambda bn: bn.weight.requires_grad and bn.bias.requires_grad      # noqa: E731
    assert [(live(getattr(bb, f'layer{li}')[0].conv3.bn), live(getattr(bb, f'layer{li}')[0].downsample.bn)) for li in range(1, 5)] \
        == [(True, True), (False, True), (True, False), (False, False)]
    assert Fn.FUSE_STAGE
    l1, g1 = _grad_step(mod, o['imgs'], o['labels'], dev)
    Fn.FUSE_STAGE = False
    try:
        l2, g2 = _grad_step(mod, o['imgs'], o['labels'], dev)
    finally:
        Fn.FUSE_STAGE = True
    assert torch.equal(l1, l2)
    assert g1.keys() == g2.keys() == {n for n, p in mod.named_parameters() if p.requires_grad}
    for n in g1:
        assert torch.equal(g1[n], g2[n]), f'{n}: stage node and block nodes differ'


class _StateOnly:
    """Stands in for the oracle where only its initial state_dict is wanted (the shared oracle has stepped since)."""

    def __init__(self, state):
        self._state = state

    def state_dict(self):
        return self._state


def _grad_step(mod, imgs, labels, dev):
    mod.zero_grad(set_to_none=True)
    loss = mod(imgs.to(dev), labels.to(dev), batch_data=None)['loss_cls']
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in mod.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('mode', ['norm_eval', 'partial_bn'])
def test_stage_node_block_nodes_and_reruns_agree_bit_for_bit(mode, dev):
    """No atomics and one arithmetic per block whichever node runs it: a stage as one autograd node, the same stage block by
    block, and a second run of either give the same bits."""
    from bdvcil_amd import functional as Fn
    ref, cfg = _oracle_only(50, 'SimpleLinear', 'CrossEntropyLoss', K=K_, seed=2, want_cfg=True)
    mod = _hip_model(ref, cfg, MODES[mode], dev)
    imgs, labels = _clips(2, 8, 64, K_, seed=8)
    mod.train()
    assert Fn.FUSE_STAGE
    l1, g1 = _grad_step(mod, imgs, labels, dev)
    l2, g2 = _grad_step(mod, imgs, labels, dev)
    Fn.FUSE_STAGE = False
    try:
        l3, g3 = _grad_step(mod, imgs, labels, dev)
    finally:
        Fn.FUSE_STAGE = True
    assert torch.equal(l1, l2) and torch.equal(l1, l3)
    assert g1.keys() == g2.keys() == g3.keys() and len(g1) > 10
    for n in g1:
        assert torch.equal(g1[n], g2[n]), f'{n}: two runs differ'
        assert torch.equal(g1[n], g3[n]), f'{n}: stage node and block nodes differ'


def test_a_block_with_mixed_batchnorm_modes_raises(dev):
    ref, cfg = _oracle_only(18, 'SimpleLinear', 'CrossEntropyLoss', K=K_, want_cfg=True)
    mod = _hip_model(ref, cfg, {}, dev)
    imgs, labels = _clips(1, 8, 64, K_)
    mod.train()
    mod.backbone.layer2[0].conv2.bn.eval()
    with pytest.raises(ValueError, match=r'layer2\.0'):
        mod(imgs.to(dev), labels.to(dev), batch_data=None)


def test_bf16_storage_keeps_raising_a_clear_error(dev):
    from bdvcil_amd import kernels as K
    ref, cfg = _oracle_only(18, 'SimpleLinear', 'CrossEntropyLoss', K=K_, want_cfg=True)
    mod = _hip_model(ref, cfg, dict(norm_eval=True), dev)
    imgs, labels = _clips(1, 8, 64, K_)
    mod.train()
    prev = K.set_conv_arith('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16 activation storage'):
            mod(imgs.to(dev), labels.to(dev), batch_data=None)['loss_cls'].backward()
    finally:
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev


def test_inference_keeps_the_fused_eval_kernels(dev):
    """Under ``torch.no_grad()`` an eval-mode model with trainable parameters runs the forward-only fused kernels, not the
    differentiable form: no ReLU sign bits are written, the logits equal bit for bit those of the same model with every parameter
    frozen (which never had another form), and bf16 activation storage runs it without raising."""
    from bdvcil_amd import functional as Fn
    from bdvcil_amd import kernels as K
    ref, cfg = _oracle_only(18, 'SimpleLinear', 'CrossEntropyLoss', K=K_, want_cfg=True)
    mod = _hip_model(ref, cfg, {}, dev)
    imgs, _ = _clips(1, 8, 64, K_)
    mod.eval()
    mod.test_cfg['average_clips'] = 'score'
    Fn.RELU_MASK_TAP = taps = []
    try:
        with torch.no_grad():
            live = mod.forward_test(imgs.to(dev))
    finally:
        Fn.RELU_MASK_TAP = None
    assert not taps
    for p in mod.parameters():
        p.requires_grad = False
    with torch.no_grad():
        frozen = mod.forward_test(imgs.to(dev))
    assert torch.equal(live, frozen)
    for p in mod.parameters():
        p.requires_grad = True
    prev = K.set_conv_arith('bf16')
    try:
        with torch.no_grad():
            low = mod.forward_test(imgs.to(dev))
    finally:
        K.set_conv_arith('bf16x3')
        K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev
    assert torch.isfinite(low).all()


def test_optimizer_step_under_partial_bn(dev):
    """The reference's parameter groups on a partial_bn model: the BatchNorm group is the stem's two tensors, a clipped step moves
    no frozen tensor and moves the others as the oracle's SGD does."""
    import bdvcil_amd as bd
    ref, cfg = _oracle_only(18, 'SimpleLinear', 'CrossEntropyLoss', K=K_, want_cfg=True)
    mod = _hip_model(ref, cfg, MODES['partial_bn'], dev)
    imgs, labels = _clips(2, 8, 64, K_, seed=5)
    _set_oracle_mode(ref, **MODES['partial_bn'])
    mod.train()
    ref(imgs, labels)['loss_cls'].backward()
    mod(imgs.to(dev), labels.to(dev), batch_data=None)['loss_cls'].backward()
    oopt = bd.build_optimizer(mod, OPT_CFG)
    stem_bn = mod.backbone.conv1.bn
    bn_groups = [g for g in oopt.param_groups if any(p is stem_bn.weight for p in g['params'])]
    assert len(bn_groups) == 1 and {id(p) for p in bn_groups[0]['params']} == {id(stem_bn.weight), id(stem_bn.bias)}
    assert bn_groups[0]['weight_decay'] == 0
    held = {id(p) for g in oopt.param_groups for p in g['params']}
    bn_params = {id(p) for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d) for p in m.parameters()}
    assert held & bn_params == {id(stem_bn.weight), id(stem_bn.bias)}
    ropt = O.build_sgd(ref)
    rp, op = dict(ref.named_parameters()), dict(mod.named_parameters())
    before = {n: p.detach().clone() for n, p in rp.items()}
    before_hip = {n: p.detach().clone() for n, p in op.items()}
    torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.grad is not None], 1.0)
    ropt.step()
    oopt.clip_grad_norm_(1.0)
    oopt.step()
    torch.cuda.synchronize()
    moved = 0
    for name, p in rp.items():
        if not p.requires_grad:
            assert torch.equal(op[name].detach(), before_hip[name]), f'{name} is frozen and moved'
            continue
        moved += 1
        assert not torch.equal(op[name].detach(), before_hip[name]), name
        assert _rel(op[name], p) <= 1e-4 or _rel_l2(op[name].detach().cpu() - before[name], p.detach() - before[name]) <= 5e-2, name
    assert moved == 2 + 20 + 2          # stem BatchNorm, the 20 conv filters of R18, the classifier's weight and bias


def test_i3d_train_step_with_norm_eval(dev):
    """``ResNet3d(norm_eval=True)`` at the smallest clip of tests/test_i3d_gpu.py's train step, against the I3D oracle with its
    BatchNorms in eval mode, under that file's gradient rule (3 * e_f32 + 1e-4 without a flip behind, + 3e-2 with one)."""
    from bdvcil_amd import functional as Fn
    from test_i3d_gpu import _cfg, _count_pool2_flips, _frames, _i3d_site_owners, _pair, _ReluRecorder3d
    import bdvcil_amd as bd
    T, S, B, Kc = 8, 64, 2, 9
    ref, _ = _pair(Kc, torch.device('cpu'), seed=2)
    cfg = _cfg(Kc)
    cfg['backbone']['norm_eval'] = True
    mod = bd.build_model(cfg)
    mod.load_state_dict(ref.state_dict())
    mod = mod.to(dev)
    ref64 = copy.deepcopy(ref).double()
    gen = torch.Generator().manual_seed(7)
    imgs = torch.randn(B, 1, 3, T, S, S, generator=gen)
    labels = torch.randint(0, Kc, (B, 1), generator=gen)
    for m in (ref, ref64):
        m.train()
        for b in m.modules():
            if isinstance(b, torch.nn.BatchNorm3d):
                b.eval()
    mod.train()
    assert not any(b.training for b in mod.modules() if isinstance(b, torch.nn.BatchNorm3d))
    buffers_before = {n: b.detach().clone() for n, b in mod.named_buffers()}
    with _ReluRecorder3d() as rec32:
        rl = ref(imgs, labels)
    rl['loss_cls'].backward()
    with _ReluRecorder3d() as rec:
        r64 = ref64(imgs.double(), labels)
    r64['loss_cls'].backward()
    Fn.RELU_MASK_TAP = taps = []
    Fn.POOL_IDX_TAP = pools = []
    try:
        ol = mod(imgs.to(dev), labels.to(dev))
    finally:
        Fn.RELU_MASK_TAP = Fn.POOL_IDX_TAP = None
    ol['loss_cls'].backward()
    torch.cuda.synchronize()
    l64 = r64['loss_cls'].item()
    assert abs(ol['loss_cls'].item() - l64) <= 3 * abs(rl['loss_cls'].item() - l64) + 1e-4 * max(1.0, abs(l64))
    pre64, pre32 = [_frames(p) for p in rec.pre], [_frames(p) for p in rec32.pre]
    flips, _ = count_relu_flips(pre64, pre32, taps)
    owners = _i3d_site_owners(ref)
    assert len(owners) == len(flips) == 1 + 3 * 16
    last_flip = max([k for k, n in enumerate(flips) if n], default=-1)
    Bc, C0, To, H0, W0 = rec.pre[0].shape
    even = lambda t: t[:, :, 0::2].permute(0, 2, 1, 3, 4).reshape(-1, C0, H0, W0)      # noqa: E731
    if count_pool_flips(even(rec.pre[0]), even(rec32.pre[0]), pools[0]):
        last_flip = max(last_flip, 0)
    if _count_pool2_flips(rec.pre[9], rec32.pre[9], pools[1]):
        last_flip = max(last_flip, 9)

    def behind_a_flip(name):
        for k, prefixes in enumerate(owners):
            if any(name.startswith(q) for q in prefixes):
                return k <= last_flip
        return False
    r64p, op = dict(ref64.named_parameters()), dict(mod.named_parameters())
    for name, p in ref.named_parameters():
        assert op[name].grad is not None, name
        e_hip, e_f32 = _rel_l2(op[name].grad, r64p[name].grad), _rel_l2(p.grad, r64p[name].grad)
        loose = behind_a_flip(name)
        print(f'{name}: relL2 hip {e_hip:.3e}, fp32 CPU {e_f32:.3e}')
        assert e_hip <= 3 * e_f32 + (3e-2 if loose else 1e-4), (name, e_hip, e_f32, loose, flips)
    for name, b in mod.named_buffers():
        assert torch.equal(b, buffers_before[name]), name
