"""Mixed-resolution batches on the GPU: the two descriptor-driven kernels against the oracles of their dense counterparts
(``bdv_resize_linear_ragged_u8`` bit-equal to oracle/resize_oracle.py, ``bdv_crop_normalize_ragged_u8`` against numpy), the packed
decode against Pillow, ``RawFrameClipLoader(ragged='always')`` bit-equal to the dense path on same-size batches (same draws, same
bits), mixed-size batches of every phase against the stages composed per sample on the CPU, and a two-task ``CILTaskLoop`` run
from a mixed-size frame tree with and without the prefetcher.  Frames of a few thousand pixels throughout."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as A
from oracle import resize_oracle as R
from test_jpeg_cpu import _picture

pytestmark = pytest.mark.gpu

MEAN = np.array([123.675, 116.28, 103.53], dtype=np.float32)
STD = np.array([58.395, 57.12, 57.375], dtype=np.float32)
# H x W sources (short_edge 32): one size group with scattered rows (48x64 twice, not adjacent), a wider clip, portrait (the short
# edge is the width, Hr varies), no multiple of the MCU, the exact-2x box mean (64x96 -> 32x48), the copy (32x40 stays), odd pixel
# counts (17x23: frames not 4-byte aligned, clips padded apart)
SIZES = [(48, 64), (48, 88), (72, 40), (48, 64), (50, 50), (64, 96), (32, 40), (17, 23)]
SMALL = dict(short_edge=32, input_size=24, bg_resize=32, test_crop=('TenCrop', 32), threads=4)


def _norm(a):
    """(T, H, W, 3) uint8 -> (T, 3, H, W) fp32, the arithmetic of the kernels: (x - mean) * (1 / std) in single precision."""
    return ((a.astype(np.float32) - MEAN) * (np.float32(1) / STD)).transpose(0, 3, 1, 2)


def _pack(clips, dev):
    """A list of (T, H, W, 3) uint8 arrays -> RaggedClips on the device."""
    from bdvcil_amd.decode import RaggedClips, RaggedLayout
    rc = RaggedClips(RaggedLayout([c.shape[1:3] for c in clips], clips[0].shape[0]), device=dev)
    rc.buffer.fill_(0xA5)
    for b, c in enumerate(clips):
        rc.clip(b).copy_(torch.from_numpy(c).to(dev))
    return rc


def _modes(table):
    """The per-clip mode the kernel picks (0 resample, 1 copy, 2 box mean), from the table's box and destination columns."""
    return {1 if (w, h) == (wd, hd) else 2 if (w, h) == (2 * wd, 2 * hd) else 0 for w, h, hd, wd in table[:, [5, 6, 8, 9]].tolist()}


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def test_resize_into_a_ragged_buffer_equals_the_oracle(dev):
    """Resize(-1, 32) of the whole frames: resample, copy and box mean in one launch; nothing is written between the clips."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd.decode import RaggedClips, plan_resize_stage, rescale_size
    T = 3
    rng = np.random.default_rng(11)
    clips = [rng.integers(0, 256, (T, h, w, 3)).astype(np.uint8) for h, w in SIZES]
    src = _pack(clips, dev)
    layout, table = plan_resize_stage(src.layout, out_sizes=[rescale_size(w, h, (-1, 32))[::-1] for h, w in SIZES])
    assert _modes(table) == {0, 1, 2}
    dst = RaggedClips(layout, device=dev)
    dst.buffer.fill_(0xA5)
    K.resize_linear_ragged_u8(src.buffer, table, T, dst.buffer)
    used = np.zeros(layout.nbytes, bool)
    for b, c in enumerate(clips):
        hd, wd = layout.sizes[b]
        got = dst.clip(b).cpu().numpy()
        for t in range(T):
            assert np.array_equal(got[t], R.resize_linear_u8(c[t], wd, hd)), (b, t)
        used[layout.offsets[b]:layout.offsets[b] + layout.clip_bytes(b)] = True
    assert (~used).any() and (dst.buffer.cpu().numpy()[~used] == 0xA5).all()


def test_crop_boxes_into_the_uniform_batch_equal_the_oracle(dev):
    """MultiScaleCrop + Resize(24): one drawn box per clip from its own size, the dense (B, T, 24, 24, 3) tensor in sample order."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError
    from bdvcil_amd.decode import plan_resize_stage
    from bdvcil_amd.frontend import MultiScaleCropResize
    T = 8
    rng = np.random.default_rng(12)
    clips = [rng.integers(0, 256, (T, h, w, 3)).astype(np.uint8) for h, w in SIZES]
    src = _pack(clips, dev)
    msc = MultiScaleCropResize(input_size=24, num_fixed_crops=13, draws=3)
    boxes = [msc.draw(w, h) for h, w in SIZES]
    boxes[1], boxes[5] = (3, 5, 24, 24), (10, 8, 48, 48)              # the copy and the box mean among the resampled ones
    _, table = plan_resize_stage(src.layout, boxes=boxes, uniform=(24, 24))
    assert _modes(table) == {0, 1, 2}
    out = torch.empty(len(SIZES), T, 24, 24, 3, dtype=torch.uint8, device=dev)
    got = K.resize_linear_ragged_u8(src.buffer, table, T, out).cpu().numpy()
    for b, (x, y, w, h) in enumerate(boxes):
        for t in range(T):
            assert np.array_equal(got[b, t], R.resize_linear_u8(clips[b][t, y:y + h, x:x + w], 24, 24)), (b, t)
    out2, _ = msc(src, boxes=boxes)                                       # the stage itself, same boxes
    assert torch.equal(out2, out) and msc.last_boxes == boxes
    bad = table.copy()
    bad[7, 3] = 20                                                        # 17 x 23 frame, x 20 + w > 23
    with pytest.raises(HipExtensionError, match='clip 7.*leaves the'):
        K.resize_linear_ragged_u8(src.buffer, bad, T, out)


@pytest.mark.parametrize('kind,crop', [('CenterCrop', 24), ('ThreeCrop', 32), ('TenCrop', 32)])
def test_crop_normalize_equals_numpy(kind, crop, dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd.frontend import crop_offsets
    T = 3
    sizes = [(32, 43), (32, 59), (58, 32), (32, 43), (32, 32), (32, 48), (32, 40)]      # SIZES after Resize(-1, 32)
    rng = np.random.default_rng(13)
    clips = [rng.integers(0, 256, (T, h, w, 3)).astype(np.uint8) for h, w in sizes]
    src = _pack(clips, dev)
    crops = [crop_offsets(kind, h, w, crop, crop) for h, w in sizes]
    assert len({tuple(c) for c in crops}) > 1                             # the offsets do depend on the clip
    o4, oc = K.crop_normalize_ragged_u8(src.buffer, src.layout.table(), T, crops, crop, crop, MEAN, STD, True, True)
    n = len(crops[0])
    assert tuple(oc.shape) == (len(sizes), n * T, 3, crop, crop) and tuple(o4.shape) == (len(sizes) * n * T, crop, crop, 4)
    oc, o4 = oc.cpu().numpy(), o4.cpu().numpy().reshape(len(sizes), n * T, crop, crop, 4)
    for b, c in enumerate(clips):
        want = _norm(np.stack(A.crop_frames(list(c), kind, crop)))       # crop-major, flips right after their crop
        assert np.abs(oc[b] - want).max() <= 1e-5, b
        assert np.abs(o4[b][..., :3].transpose(0, 3, 1, 2) - want).max() <= 1e-5 and (o4[b][..., 3] == 0).all(), b


# ---- frames on disk ------------------------------------------------------------------------------------------------------------------
def _video(root, name, h, w, n, kind, rng, subsampling, label):
    from PIL import Image
    d = root / name
    d.mkdir(parents=True)
    base = _picture(h, w, kind, rng)
    for i in range(1, n + 1):
        Image.fromarray(np.roll(base, (i, 2 * i), axis=(0, 1))).save(str(d / f'img_{i:05}.jpg'), quality=85, subsampling=subsampling)
    return {'frame_dir': str(d), 'total_frames': n, 'label': label}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """One video per entry of SIZES (9 - 12 frames; 4:2:0 and 4:4:4 alternate, so the 48 x 64 group mixes samplings), four videos
    each of 48 x 88 (clips dense in the packed buffer) and 50 x 50 (clips padded apart), two backgrounds."""
    from PIL import Image
    root = tmp_path_factory.mktemp('ragged_frames')
    rng = np.random.default_rng(31)
    mixed = [_video(root, f'mixed_{k}', h, w, 9 + k % 4, k % 2, rng, (2, 2, 0, 0)[k % 4], k) for k, (h, w) in enumerate(SIZES)]
    same = {hw: [_video(root, f'same_{hw[0]}x{hw[1]}_{k}', *hw, 10 + k, k % 2, rng, 2, k) for k in range(4)] for hw in ((48, 88), (50, 50))}
    bgs = []
    for k, (h, w) in enumerate(((40, 60), (45, 50))):
        p = root / f'bg_{k}.jpg'
        Image.fromarray(_picture(h, w, k, rng)).save(str(p), quality=90)
        bgs.append(str(p))
    return dict(mixed=mixed, same=same, bgs=bgs)


_DECODED = {}


def _pillow(info, i):
    """Frame i of a video as Pillow decodes it; kept, every test below reads the same few files."""
    from PIL import Image
    key = (info['frame_dir'], int(i))
    if key not in _DECODED:
        _DECODED[key] = np.asarray(Image.open(os.path.join(info['frame_dir'], f'img_{int(i):05}.jpg')).convert('RGB'))
    return _DECODED[key]


def _resized_clip(info, inds):
    """Pillow decode -> Resize(-1, 32) by the oracle: (T, Hr, Wr, 3) uint8."""
    out = []
    for i in inds:
        img = _pillow(info, i)
        Wr, Hr = R.rescale_size(img.shape[1], img.shape[0], (-1, 32))
        out.append(R.resize_linear_u8(img, Wr, Hr))
    return np.stack(out)


@pytest.mark.parametrize('picks', [list(range(8)), [7, 0, 7], [3]], ids=['table', 'padded_group', 'one_clip'])
def test_decode_clips_ragged_equals_pillow(tree, picks, dev):
    from bdvcil_amd.decode import JpegDecoder
    infos = [tree['mixed'][k] for k in picks]
    T = 3
    clips = [[open(os.path.join(v['frame_dir'], f'img_{i:05}.jpg'), 'rb').read() for i in (1, 4, 9)] for v in infos]
    rc = JpegDecoder(dev, threads=4).decode_clips_ragged(clips)
    assert rc.sizes == [SIZES[k] for k in picks] and rc.T == T and len(rc) == len(picks)
    for b, v in enumerate(infos):
        got = rc.clip(b).cpu().numpy()
        for t, i in enumerate((1, 4, 9)):
            assert np.array_equal(got[t], _pillow(v, i)), (b, t)
    for g, rows in enumerate(rc.layout.rows):                             # the group views show the same clips
        assert tuple(rc.groups[g].shape) == (len(rows), T, *rc.layout.groups[g], 3)
        for r, b in enumerate(rows):
            assert torch.equal(rc.groups[g][r], rc.clip(b))
    with pytest.raises(ValueError, match='different lengths'):
        JpegDecoder(dev).decode_clips_ragged([clips[0], clips[0][:2]])
    if picks[:4] == [0, 1, 2, 3]:       # one clip whose frames change sampling (4:2:0, 4:4:4, 4:2:0) at one size: parsed stream by stream
        rc = JpegDecoder(dev).decode_clips_ragged([clips[1], [clips[0][0], clips[3][1], clips[0][2]]])
        want = [_pillow(infos[0], 1), _pillow(infos[3], 4), _pillow(infos[0], 9)]
        assert all(np.array_equal(rc.clip(1)[t].cpu().numpy(), want[t]) for t in range(T))
    if len(picks) > 1:
        with pytest.raises(ValueError, match='different sizes'):           # the dense entry point keeps its rule
            JpegDecoder(dev).decode_clips(clips)
        with pytest.raises(ValueError, match='clip 0 has frames of different sizes'):
            JpegDecoder(dev).decode_clips_ragged([[clips[0][0], clips[1][0], clips[0][1]]])


# ---- same-size batches: the packed path returns the dense path's bits ------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(48, 88), (50, 50)], ids=['dense_clips', 'padded_clips'])
def test_ragged_always_equals_the_dense_path_on_same_size_batches(tree, hw, dev):
    """The configs' train settings (RandAugment 0.75, background mix for the samples it skipped) and the three eval phases; the
    generators are left in the same state."""
    from bdvcil_amd.decode import RawFrameClipLoader
    infos = tree['same'][hw]
    seen_aug = seen_mixed = False
    for seed in (1, 2, 3):
        a = RawFrameClipLoader(dev, bg_files=tree['bgs'], seed=seed, **SMALL)
        b = RawFrameClipLoader(dev, bg_files=tree['bgs'], seed=seed, ragged='always', **SMALL)
        for phase in ('train', 'val', 'train', 'features_extraction', 'test'):
            x, y = a(infos, phase), b(infos, phase)
            assert x.keys() == y.keys()
            assert torch.equal(x['imgs'], y['imgs']) and torch.equal(x['frame_inds'], y['frame_inds']), (seed, phase)
            if phase == 'train':
                assert torch.equal(x['randAug'], y['randAug'])
                assert a.train_front.crop_resize.last_boxes == b.train_front.crop_resize.last_boxes
                seen_aug |= bool(x['randAug'].any())
                seen_mixed |= bool((~x['randAug']).any())
        assert tuple(x['imgs'].shape) == (4, 80, 3, 32, 32)
        assert a.draws.py.random() == b.draws.py.random() and a.draws.np.random_sample() == b.draws.np.random_sample()
        assert a.draws.randint(1 << 30) == b.draws.randint(1 << 30)
    assert seen_aug and seen_mixed


# ---- mixed-size batches against the stages composed per sample -----------------------------------------------------------------------
BATCHES = {'table': list(range(8)), 'one_clip': [2], 'all_distinct': [1, 2, 4, 5, 6, 7], 'abab': [0, 1, 3, 1]}


@pytest.mark.parametrize('name', list(BATCHES))
@pytest.mark.parametrize('T', [3, 8])
def test_mixed_batch_eval_phases(tree, name, T, dev):
    from bdvcil_amd.decode import RawFrameClipLoader
    infos = [tree['mixed'][k] for k in BATCHES[name]]
    loader = RawFrameClipLoader(dev, num_segments=T, **SMALL)
    for phase, kind, crop in (('val', 'CenterCrop', 24), ('features_extraction', 'CenterCrop', 24), ('test', 'TenCrop', 32)):
        batch = loader(infos, phase)
        n = 10 if kind == 'TenCrop' else 1
        assert tuple(batch['imgs'].shape) == (len(infos), n * T, 3, crop, crop)
        assert batch['label'].tolist() == [[v['label']] for v in infos]
        for k, v in enumerate(infos):
            inds = R.sample_frames(v['total_frames'], T, test_mode=True)
            assert batch['frame_inds'][k].tolist() == inds.tolist()
            want = _norm(np.stack(A.crop_frames(list(_resized_clip(v, inds)), kind, crop)))
            assert np.abs(batch['imgs'][k].cpu().numpy() - want).max() <= 1e-5, (phase, k)


def test_mixed_batch_raises_without_the_ragged_path(tree, dev):
    """What the loader did before: the dense decode refuses a batch that mixes sizes."""
    from bdvcil_amd.decode import RawFrameClipLoader
    loader = RawFrameClipLoader(dev, **SMALL)
    clips, _ = loader._clips(tree['mixed'][:2], test_mode=True)
    with pytest.raises(ValueError, match='different sizes'):
        loader._resized(clips)
    with pytest.raises(ValueError, match='ragged'):
        RawFrameClipLoader(dev, ragged='never', **SMALL)


def _train_reference(loader, batch, infos, draws=None):
    """Per sample: decode -> Resize -> (the recorded RandAugment draws through the oracle) -> the recorded box -> Resize(24) -> Normalize."""
    boxes = loader.train_front.crop_resize.last_boxes
    assert len(boxes) == len(infos)
    for k, v in enumerate(infos):
        clip = list(_resized_clip(v, batch['frame_inds'][k].tolist()))
        if draws is not None:
            ops, flip_sign, init_loc = draws[k]
            for op, minval, maxval in ops:
                val = (float(10) / 30) * float(maxval - minval) + minval
                clip = [A.apply_op(op, f, val, flip_sign, init_loc) for f in clip]
        x, y, w, h = boxes[k]
        assert 0 <= x and x + w <= clip[0].shape[1] and 0 <= y and y + h <= clip[0].shape[0]     # drawn from this sample's own size
        want = _norm(np.stack([R.resize_linear_u8(f[y:y + h, x:x + w], 24, 24) for f in clip]))
        assert np.abs(batch['imgs'][k].cpu().numpy() - want).max() <= 1e-5, k


def test_mixed_batch_train_phase(tree, dev):
    from bdvcil_amd.decode import RawFrameClipLoader
    infos = tree['mixed']
    # (1) RandAugment never fires, alpha = 0: decode -> Resize -> MultiScaleCrop -> Resize(24) -> Normalize, backgrounds read and unused
    loader = RawFrameClipLoader(dev, randAug=dict(n=2, m=10, prob=0.0), alpha=0.0, bg_files=tree['bgs'], seed=5, **SMALL)
    batch = loader(infos, 'train')
    assert tuple(batch['imgs'].shape) == (8, 8, 3, 24, 24) and not batch['randAug'].any()
    assert loader.train_front.randaug.last_draws == [None] * 8
    _train_reference(loader, batch, infos)
    # (2) RandAugment always fires, no background mix: the recorded per-sample draws through the oracle
    loader = RawFrameClipLoader(dev, randAug=dict(n=2, m=10, prob=2), bg_mix=False, seed=6, **SMALL)
    names = set()
    for _ in range(2):
        batch = loader(infos, 'train')
        draws = loader.train_front.randaug.last_draws
        assert batch['randAug'].all() and len(draws) == 8 and all(d is not None for d in draws)
        _train_reference(loader, batch, infos, draws)
        names |= {op[0] for d in draws for op in d[0]}
    assert len(names) >= 6                                                # a spread of operations, geometric and per-frame-table ones
    # (3) the configs' settings on a mixed batch: both branches occur, everything finite
    loader = RawFrameClipLoader(dev, bg_files=tree['bgs'], seed=7, **SMALL)
    flags = torch.stack([loader(infos, 'train')['randAug'] for _ in range(3)])
    batch = loader(infos, 'train')
    assert torch.isfinite(batch['imgs']).all() and flags.any() and (~flags).any()


# ---- through the loop ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loop_runs(tmp_path_factory):
    """Two tasks of two classes, TSM-R18 at 64 x 64, one epoch each, from frames 36 high and 48 - 63 wide (every batch mixes sizes):
    once with the loader called inline and once two batches ahead."""
    import bdvcil_amd.heads
    import bdvcil_amd.task_loop as TL
    from bdvcil_amd.decode import RawFrameClipLoader
    from test_task_loop_gpu import _config
    root = tmp_path_factory.mktemp('ragged_loop')
    rng = np.random.default_rng(41)
    lines = {'train': [], 'val': []}
    for label in range(4):
        for name, n in (('train', 3), ('val', 1)):
            for k in range(n):
                rel = f'class{label}/{name}_v{label}_{k}'
                _video(root / 'rawframes', rel, 36, (48, 52, 56, 63)[(label + k) % 4], 12, (label + k) % 2, rng, 2, label)
                lines[name].append(f'{rel} 12 {label}\n')
    for name in lines:
        (root / f'{name}.txt').write_text(''.join(lines[name]))
    bg = root / 'bg_0.jpg'
    from PIL import Image
    Image.fromarray(_picture(80, 90, 1, rng)).save(str(bg), quality=85)
    out = {}
    for prefetch in (0, 2):
        run = root / f'prefetch_{prefetch}'
        run.mkdir()
        random.seed(11); np.random.seed(11); torch.manual_seed(11)      # model initialisation and the dropout masks' seed
        bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0
        loader = RawFrameClipLoader('cuda', bg_files=[str(bg)], seed=7, short_edge=72, input_size=64, bg_resize=72, test_crop=('TenCrop', 72),
                                    threads=4)
        cfg = _config(run, task_splits=[[0, 1], [2, 3]], ending_task=1, num_epochs_per_task=1, videos_per_gpu=4, testing_videos_per_gpu=4,
                      data_root=str(root / 'rawframes'), train_ann_file=str(root / 'train.txt'), val_ann_file=str(root / 'val.txt'))
        loop = TL.CILTaskLoop(cfg, loader, device='cuda', seed=0, log=lambda *a: None, prefetch=prefetch)
        history = loop.train()
        loop.close()
        work = run / 'work'
        out[prefetch] = dict(tasks=[h['task'] for h in history],
                             ckpt=[torch.load(work / 'ckpt' / f'ckpt_task_{t}.pt', map_location='cpu', weights_only=True) for t in range(2)],
                             exemplar=[(work / 'exemplar' / f'exemplar_task_{t}.txt').read_text() for t in range(2)])
    return out


def test_two_tasks_from_a_mixed_size_tree(loop_runs):
    off, on = loop_runs[0], loop_runs[2]
    assert off['tasks'] == on['tasks'] == [0, 1]
    for t in range(2):
        assert off['ckpt'][t].keys() == on['ckpt'][t].keys() and len(off['ckpt'][t]) > 50
        for k, v in off['ckpt'][t].items():
            assert torch.equal(v, on['ckpt'][t][k]), (t, k)
            assert not v.is_floating_point() or torch.isfinite(v).all(), (t, k)
        assert off['exemplar'][t] == on['exemplar'][t] and off['exemplar'][t].strip()
