"""Foreground merging on the device (csrc/fg_merge.hip), stage by stage against the fp64 restatement (tests/fg_merge_oracle.py), in
every layout where a stage reads the clip; each stage is fed the GPU's own output of the stage before it, so no test hangs on a
threshold falling between two roundings.  Then the whole chain on the two-halves scene, the blending through a recognizer, and the
``fg_merge`` key of ``CILTaskLoop`` under the three methods."""
import copy
import functools

import numpy as np
import pytest
import torch

import fg_merge_oracle as FO

pytestmark = pytest.mark.gpu

MOTION_SHAPES = [(3, 3, 20, 20), (2, 4, 13, 19), (2, 2, 16, 24), (1, 8, 224, 224)]
LAYOUTS = ('tchw', 'thwc4', 'cthw')


def _K():
    import bdvcil_amd as bd
    return bd.kernels


def _to_dev(x, layout, dev):
    """A planar host clip batch -> (device storage in ``layout``, the wrapped object the blending takes)."""
    import bdvcil_amd as bd
    B, T = x.shape[:2]
    if layout == 'tchw':
        d = x.to(dev).contiguous()
        return d, d
    if layout == 'thwc4':
        d = FO.to_nhwc4(x).to(dev).contiguous()
        return d, bd.Nhwc4Frames(d, B, T)
    d = FO.to_cthw(x).to(dev).contiguous()
    return d, d


def _to_host(d, layout, B, T):
    d = d.cpu()
    if layout == 'tchw':
        return d
    if layout == 'thwc4':
        return FO.from_nhwc4(d, B, T)
    return d[:, 0].permute(0, 2, 1, 3, 4).contiguous()


def _u32(t):
    return t.cpu().long() & 0xffffffff


@functools.lru_cache(maxsize=None)
def _motion_case(i):
    x = FO.random_clip(*MOTION_SHAPES[i], seed=i)
    return x, FO.motion_q(x, torch.float64)


# ---- stages 1-3 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('i', range(len(MOTION_SHAPES)), ids=[str(s) for s in MOTION_SHAPES])
def test_motion_blur_quantise(i, layout, dev):
    B, T, H, W = MOTION_SHAPES[i]
    x, (q64, g64, d64) = _motion_case(i)
    data, _ = _to_dev(x, layout, dev)
    q, g, d = _K().fg_motion_q(data, B, T, H, W, layout)
    k = FO.tap_count(H, W)
    assert k == (23 if H == 224 else 3 if H == 20 else 1)
    # relative: every term is non-negative.  3 (T - 1) additions of rounded differences, 2 k products and sums, the division and the
    # fp32 taps: (3 (T - 1) + 2 k + 8) units of 2^-24 cover both maps
    rel_d = rel_g = (3 * (T - 1) + 2 * k + 8) * 2.0 ** -24
    ed = ((d.cpu().double() - d64).abs() - rel_d * d64).max().item()
    eg = ((g.cpu().double() - g64).abs() - rel_g * g64).max().item()
    dq = (q.cpu().int() - q64.int()).abs()
    print(f'{MOTION_SHAPES[i]} {layout}: d excess {ed:.3e}, g excess {eg:.3e}, q max diff {int(dq.max())}, share {(dq > 0).float().mean().item():.5f}')
    assert ed <= 0 and eg <= 0
    assert dq.max() <= 1 and (dq > 0).float().mean() <= 0.01
    assert q.dtype == torch.uint8 and q.shape == (B, H, W) and int(q.max()) == 255 and int(q.min()) == 0


@pytest.mark.parametrize('layout', LAYOUTS)
def test_constant_clip_has_q_zero(layout, dev):
    x = torch.full((2, 3, 3, 20, 20), 0.37)
    x[1] = FO.random_clip(1, 1, 20, 20)[0].repeat(3, 1, 1, 1)            # static, not flat
    data, _ = _to_dev(x, layout, dev)
    q, g, d = _K().fg_motion_q(data, 2, 3, 20, 20, layout)
    assert not q.any() and not g.any() and not d.any()


# ---- stages 4-5 ----------------------------------------------------------------------------------------------------------------------

def _hist_clip(B, T, H, W, seed, special):
    """Raw 8-bit values (every multiple of 256 / bins sits exactly on a bin edge after normalisation with mean 0, std 1), plus values
    far outside the colour range and a NaN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, T, 3, H, W), generator=g).float()
    if special:
        x[0, 0, 0, 0, 0] = 32.0           # an edge of bins = 8 (and of 2, 16): bin 1, not 0
        x[0, 0, 1, 0, 1] = 128.0
        x[0, 0, 2, 0, 2] = 1e30           # clamps to the last bin
        x[0, 1, 0, 1, 0] = -1e30          # clamps to bin 0
        x[0, 1, 1, 1, 1] = float('nan')   # bin 0
        x[0, 1, 2, 1, 2] = float('inf')
        x[0, 0, 0, 2, 2] = 255.999
    return x


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('shape,bins', [((2, 3, 20, 20), 8), ((2, 2, 13, 19), 2), ((2, 3, 13, 19), 16), ((2, 3, 40, 40), 8)], ids=str)
def test_histograms_exact_and_refined_map(shape, bins, layout, dev):
    B, T, H, W = shape
    K = _K()
    mean, std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    x = _hist_clip(B, T, H, W, seed=H + bins, special=True)
    lo, sc = K.fg_colour_params(bins, mean, std)
    assert sc.tolist() == [bins / 256] * 3
    data, _ = _to_dev(x, layout, dev)
    q = torch.randint(0, 256, (B, H, W), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    q[0, 0, :3] = 255
    s, F, N = K.fg_hist_refine(data, q.to(dev), B, T, H, W, layout, bins, lo, sc)
    idx = FO.bin_index(x, bins, lo, sc)
    assert int(idx[0, 0, 0, 0]) >> (2 * (bins.bit_length() - 1)) == bins // 8          # the edge value: bin 32 * bins / 256 exactly
    assert int(idx[0, 0, 0, 2]) % bins == bins - 1 and int(idx[0, 1, 1, 0]) // (bins * bins) == 0
    F64, N64 = FO.histograms(idx, q, bins)
    assert torch.equal(_u32(F), F64) and torch.equal(_u32(N), N64)
    assert int(N64.sum()) == B * T * H * W
    s64 = FO.refine(idx, F64, N64, torch.float64)
    err = (s.cpu().double() - s64).abs().max().item()
    print(f'{shape} bins {bins} {layout}: s max abs err {err:.3e} (bound {(T + 6) * 2.0 ** -24:.3e})')
    assert err <= (T + 6) * 2.0 ** -24


def test_histograms_default_colours_on_the_gpus_own_q(dev):
    """The chain closed: q from the device's stages 1-3, normalised clip, default mean / std; one 224 x 224 clip puts 49 workgroups on
    every bin."""
    K = _K()
    for i in (0, 3):
        B, T, H, W = MOTION_SHAPES[i]
        x, _ = _motion_case(i)
        for layout in ('tchw', 'thwc4'):
            data, _ = _to_dev(x, layout, dev)
            q, _, _ = K.fg_motion_q(data, B, T, H, W, layout)
            lo, sc = K.fg_colour_params(8, FO.IMG_MEAN, FO.IMG_STD)
            s, F, N = K.fg_hist_refine(data, q, B, T, H, W, layout, 8, lo, sc)
            idx = FO.bin_index(x, 8, lo, sc)
            F64, N64 = FO.histograms(idx, q.cpu(), 8)
            assert torch.equal(_u32(F), F64) and torch.equal(_u32(N), N64)
            assert (s.cpu().double() - FO.refine(idx, F64, N64, torch.float64)).abs().max() <= (T + 6) * 2.0 ** -24


# ---- stage 6 -------------------------------------------------------------------------------------------------------------------------

def _select_cases():
    g = torch.Generator().manual_seed(11)
    r = torch.rand(2, 400, generator=g)
    tie = torch.rand(2, 400, generator=g) * 0.5
    tie[:, 100:140] = 0.75                         # 40 equal values straddle k = 20
    few = torch.zeros(2, 400)
    few[0, :7] = torch.rand(7, generator=g) + 0.1  # 7 positive values, k = 200
    few[1, 5] = 1e-40                              # a single denormal
    odd = torch.rand(3, 13 * 19, generator=g)
    odd[1, ::3] = 0
    big = torch.rand(1, 224, 224, generator=g)
    big[0, 100:110] = big[0, 0, 0]
    return {'all_equal': (torch.full((2, 400), 0.25), 200), 'all_zero': (torch.zeros(2, 400), 200), 'few_positive': (few, 200),
            'tie': (tie, 20), 'k1': (r, 1), 'k_all': (r, 400), 'k_all_with_zero': (few, 400), 'odd': (odd, 123), 'odd_1025': (torch.rand(2, 1025, generator=g), 512),
            'big224': (big, 25088)}


@pytest.mark.parametrize('name', list(_select_cases()))
def test_selection_is_exact(name, dev):
    s, k = _select_cases()[name]
    v, mask, count = _K().fg_select(s.to(dev).contiguous(), k)
    rv, rmask, rcount = FO.select(s, k)
    assert torch.equal(v.cpu().view(torch.int32), rv.view(torch.int32))
    assert mask.dtype == torch.uint8 and mask.shape == s.shape and torch.equal(mask.cpu(), rmask)
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), rcount)
    if name == 'all_zero':
        assert count.tolist() == [0, 0]
    if name == 'all_equal':
        assert count.tolist() == [400, 400]
    if name == 'tie':
        assert count.tolist() == [40, 40]
    if name == 'few_positive':
        assert count.tolist() == [7, 1]


# ---- stage 7 -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('H,W', [(13, 19), (20, 20)], ids=str)
def test_merge_is_gather_then_assign(H, W, layout, dev):
    B, T = 7, 3
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, T, 3, H, W, generator=g)
    mask = (torch.rand(B, H, W, generator=g) < 0.5).to(torch.uint8)
    mask[1, :, :8] = 0                                  # long background runs: the 16-byte path
    mask[2, :, 4:] = 1
    mask[6] = 0
    count = mask.view(B, -1).sum(1).int()
    assert int(count[6]) == 0
    perm = torch.tensor([0, 2, 1, 4, 5, 3, 1])          # a fixed point, a 2-cycle, a 3-cycle; clip 6 (no foreground) reads clip 1
    apply = torch.tensor([True, True, True, True, False, True, True])
    # 4 is off although it sits in the cycle: 3 reads it directly, 5 reads 3 as it was
    data, _ = _to_dev(x, layout, dev)
    before = data.clone()
    out = _K().fg_merge_(data, mask.to(dev), count.to(dev), perm, apply, B, T, H, W, layout)
    assert out is data
    ref = FO.merge(x, mask, count, perm, apply)
    got = _to_host(data, layout, B, T)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    S = data.numel() // B
    flat, was = data.view(B, S).cpu(), before.view(B, S).cpu()
    for b in (0, 4, 6):                                  # fixed point, apply false, count == 0: bitwise untouched, fourth lane included
        assert torch.equal(flat[b].view(torch.int32), was[b].view(torch.int32))
    if layout == 'thwc4':                                # the fourth lane moves with its pixel
        lane, lane0 = data[..., 3].view(B, T, H, W).cpu(), before[..., 3].view(B, T, H, W).cpu()
        m = mask.bool().view(B, 1, H, W)
        for b, p in ((1, 2), (2, 1), (3, 4), (5, 3)):
            assert torch.equal(lane[b], torch.where(m[b], lane0[b], lane0[p]))
    for b, p in ((1, 2), (2, 1), (3, 4), (5, 3)):
        assert not torch.equal(ref[b], x[b]) or not (mask[b] == 0).any()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('shape', [(3, 3, 20, 20), (2, 4, 12, 18), (1, 8, 224, 224)], ids=str)
def test_two_halves_end_to_end(shape, layout, dev):
    import bdvcil_amd as bd
    B, T, H, W = shape
    x = FO.two_halves_scene(*shape, seed=3)
    data, imgs = _to_dev(x, layout, dev)
    seg, mask, count = bd.foreground_mask(imgs, beta=0.5, bins=8)
    left = torch.zeros((B, H, W), dtype=torch.uint8)
    left[..., :W // 2] = 1
    assert seg.shape == (B, H, W) and seg.dtype == torch.float32 and torch.equal(mask.cpu(), left) and count.tolist() == [H * (W // 2)] * B
    s64 = FO.foreground_mask(x, dtype=torch.float64)[0]
    print(f'{shape} {layout}: seg max abs diff to fp64 {(seg.cpu().double() - s64).abs().max().item():.3e}')
    if B < 2:
        return
    blend = bd.ForegroundMergeBlending(beta=0.5, prob=1.0)
    perm = torch.tensor([1, 2, 0][:B] if B == 3 else [1, 0])
    blend.draw = lambda *a: (perm, torch.ones(B, dtype=torch.bool))            # a forced draw
    label = torch.arange(B, device=dev).view(B, 1)
    before = data.clone()
    out, lab = blend(imgs, label)
    assert out is imgs and lab is label
    got, was = _to_host(data, layout, B, T), _to_host(before, layout, B, T)
    for b in range(B):
        assert torch.equal(got[b, ..., :W // 2].view(torch.int32), was[b, ..., :W // 2].view(torch.int32))
        assert torch.equal(got[b, ..., W // 2:].view(torch.int32), was[int(perm[b]), ..., W // 2:].view(torch.int32))


def test_blending_draws_and_partial_apply(dev):
    import bdvcil_amd as bd
    x = FO.two_halves_scene(4, 3, 20, 20, seed=9)
    x[3] = x[3, :1]                                          # a static clip: count == 0, never merged
    data = x.to(dev)
    blend = bd.ForegroundMergeBlending(prob=0.6)
    torch.manual_seed(21)
    perm, apply = blend.draw(4)
    torch.manual_seed(21)
    out, _ = blend(data, torch.zeros(4, 1, dtype=torch.int64, device=dev))
    assert out is data
    _, mask, count, _ = FO.foreground_mask(x)
    assert int(count[3]) == 0
    assert torch.equal(data.cpu().view(torch.int32), FO.merge(x, mask, count, perm, apply).view(torch.int32))


# ---- through the model and the loop -------------------------------------------------------------------------------------------------

def _small_model_cfg(num_classes, T=3):
    from test_task_loop_gpu import _model_cfg
    cfg = _model_cfg(num_classes)
    cfg['backbone']['num_segments'] = T
    cfg['cls_head']['num_segments'] = T
    cfg['cls_head']['dropout_ratio'] = 0.0
    return cfg


def test_blending_through_the_recognizer(dev):
    """TSM-R18, 16-class LSC head, B = 3, T = 3, 32 x 32: hard labels reach LSCLoss, the loss is finite and back-propagates."""
    import bdvcil_amd as bd
    torch.manual_seed(0)
    cfg = _small_model_cfg(16)
    cfg['train_cfg'] = dict(blending=dict(type='ForegroundMergeBlending', prob=1.0, beta=0.5, num_classes=16))
    model = bd.build_model(cfg).to(dev)
    model.train()
    assert isinstance(model.blending, bd.ForegroundMergeBlending)
    imgs = FO.two_halves_scene(3, 3, 32, 32, seed=4).to(dev)
    before = imgs.clone()
    label = torch.tensor([[3], [7], [15]], device=dev)
    out = model(imgs, label, return_loss=True)
    assert torch.isfinite(out['loss_cls']).all()
    out['loss_cls'].sum().backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and any(g.abs().sum() > 0 for g in grads)
    assert torch.equal(imgs[..., :16], before[..., :16]) and not torch.equal(imgs[..., 16:], before[..., 16:])      # merged in place


def _loop_cfg(tmp, method, **over):
    from test_task_loop_gpu import _config
    tmp.mkdir()
    cfg = _config(tmp, methods=method, ending_task=1, videos_per_gpu=3, **over)
    cfg['model'] = _small_model_cfg(2)
    if method != 'base':
        cfg['model']['cls_head']['inc_head_config'] = dict(type='SimpleLinear', out_features=2)
        cfg['model']['cls_head']['loss_cls'] = dict(type='CrossEntropyLoss')
        cfg.update(video_mix_prob=0.5, video_mix_alpha=1.0)
    return cfg


def _two_steps(tmp, method, task=0, spy=None, **over):
    """A loop on the synthetic loader (T = 3, 32 x 32), two training steps of three clips each.  -> (losses, the two batches)"""
    import random
    import bdvcil_amd.heads
    import bdvcil_amd.task_loop as TL
    torch.manual_seed(1234)
    random.seed(1234)
    np.random.seed(1234)
    bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0
    loader = TL.SyntheticClipLoader('cuda', num_segments=3, size=32, seed=5)
    loop = TL.CILTaskLoop(_loop_cfg(tmp, method, **over), loader, device='cuda', seed=0, log=lambda *a: None)
    try:
        if task == 1:                                    # as CILTaskLoop.train() moves on: the teacher is a copy with the wider head
            loop._current_task = 1
            loop.prev_model.load_state_dict(loop.current_model.state_dict())
            loop.current_model.update_fc(loop.num_classes(1))
            loop.prev_model.update_fc(loop.num_classes(1))
            loop._freeze_prev()
        if spy is not None:
            spy(loop)
        loop.current_model.train()
        losses, batches = [], []
        for batch in loop._load(loop.train_dataset, [[0, 1, 2], [3, 4, 5]]):
            out = loop._training_step(batch)
            out['loss'].backward()
            losses.append(float(out['loss'].detach()))
            batches.append(batch)
        return losses, batches, loop
    finally:
        loop.close()


@pytest.mark.parametrize('method', ['base', 'icarl', 'icarl_video_mix'])
def test_loop_runs_with_fg_merge(method, tmp_path, dev):
    import bdvcil_amd as bd
    calls = []

    def spy(loop):
        fg = loop.fg_merge
        assert isinstance(fg, bd.ForegroundMergeBlending) and (fg.beta, fg.prob, fg.bins) == (0.4, 1.0, 8)
        loop.fg_merge = lambda imgs, label: calls.append(imgs) or fg(imgs, label)
    losses, batches, loop = _two_steps(tmp_path / 'run', method, spy=spy, fg_merge=dict(beta=0.4, prob=1.0))
    assert len(losses) == 2 and np.isfinite(losses).all()
    assert len(calls) == 2 and all(c is b['imgs'] for c, b in zip(calls, batches))
    with torch.no_grad():                                                   # prediction never merges
        loop.predict(loop.train_dataset, 3, extract_repr=False)
    assert len(calls) == 2


def test_loop_prob_zero_equals_the_key_absent(tmp_path, dev):
    absent, _, la = _two_steps(tmp_path / 'absent', 'base')
    zero, _, lz = _two_steps(tmp_path / 'zero', 'base', fg_merge=dict(prob=0))
    assert la.fg_merge is None and lz.fg_merge is not None
    assert absent == zero and len(zero) == 2
    merged, _, _ = _two_steps(tmp_path / 'on', 'base', fg_merge=dict(prob=1.0))
    assert merged != absent


def test_teacher_sees_the_merged_clips(tmp_path, dev):
    seen = {}

    def spy(loop):
        fg, teacher = loop.fg_merge, loop.prev_model.forward_test

        def merge(imgs, label):
            seen.setdefault('before', []).append(imgs.clone())
            out = fg(imgs, label)
            seen.setdefault('merged', []).append(out[0])
            return out

        def forward_test(imgs, *a, **kw):
            seen.setdefault('teacher', []).append((imgs, imgs.clone()))
            return teacher(imgs, *a, **kw)
        loop.fg_merge, loop.prev_model.forward_test = merge, forward_test
    losses, batches, _ = _two_steps(tmp_path / 'run', 'base', task=1, spy=spy, fg_merge=dict(prob=1.0))
    assert np.isfinite(losses).all() and len(seen['teacher']) == 2
    for i in range(2):
        obj, value = seen['teacher'][i]
        assert obj is seen['merged'][i] and obj is batches[i]['imgs']            # by identity: the tensor merged in place
        assert not torch.equal(value, seen['before'][i])                         # and it held the merged pixels when the teacher read it
