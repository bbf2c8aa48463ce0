"""Generate golden vectors for ActorCutMix from the reference's own ``libs/pipelines/box.py`` and
``libs/loader/actor_cut_mix_loader.py``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_actor_cut_mix.py

Both files are imported by path.  Stubs stand in for what they import: no-op registries, ``Compose``, UPSTREAM mmaction2 0.24
``Resize`` / ``Flip`` bases holding only their constructor arguments, ``SampleFrames`` / ``RawFrameDecode`` / ``MultiScaleCrop``
(UPSTREAM semantics, from oracle/resize_oracle.py), and ``mmcv.imresize`` / ``rescale_size`` / ``imflip_`` (cv2 is absent: the
resampling calls oracle/resize_oracle.py, the flip is an in-place ``np.flip``).  The reference's DetectionLoad, ResizeWithBox,
FlipWithBox, BuildHumanMask, SceneCutOut, ActorCutOut, ``actor_cut_mix`` and ``_calc_foreground_ratio`` then run as written, at
small scales ((-1, 40) -> (32, 32), T = 4).  Written to ``tests/golden/actor_cut_mix_golden.npz``: the synthetic frames and
detections, per sample the draws, the final int boxes, the mask, the composite and the ratio; and a seeded sequence of whole
``prepare_train_frames`` calls (acm_prob 0.5, the RandAugment branch included) with the draws each sample made.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import resize_oracle as R  # noqa: E402

OUT = os.path.join(HERE, 'actor_cut_mix_golden.npz')
T, SHORT, OUT_HW, THRES = 4, 40, 32, 0.4


class _NoopRegistry:
    def register_module(self, *a, **k):
        return lambda cls: cls


class _Resize:
    """UPSTREAM mmaction2 0.24 ``Resize.__init__`` (the base ResizeWithBox derives from): only the constructor arguments."""

    def __init__(self, scale, keep_ratio=True, interpolation='bilinear', lazy=False):
        if isinstance(scale, tuple):
            max_long_edge, max_short_edge = max(scale), min(scale)
            if max_short_edge == -1:
                scale = (np.inf, max_long_edge)
        self.scale, self.keep_ratio, self.interpolation, self.lazy = scale, keep_ratio, interpolation, lazy

    def __call__(self, results):            # plain Resize (the RandAugment branch)
        img_h, img_w = results['img_shape']
        new_w, new_h = _rescale_size((img_w, img_h), self.scale) if self.keep_ratio else self.scale
        results['imgs'] = [R.resize_linear_u8(img, new_w, new_h) for img in results['imgs']]
        results['img_shape'] = (new_h, new_w)
        return results


class _Flip:
    """UPSTREAM mmaction2 0.24 ``Flip.__init__``: only the constructor arguments."""

    def __init__(self, flip_ratio=0.5, direction='horizontal', flip_label_map=None, left_kp=None, right_kp=None, lazy=False):
        self.flip_ratio, self.direction, self.flip_label_map, self.lazy = flip_ratio, direction, flip_label_map, lazy


def _rescale_size(old_size, scale):
    """UPSTREAM ``mmcv.rescale_size`` for a tuple scale: factor min(long / max(h, w), short / min(h, w)), int(x * f + 0.5)."""
    w, h = old_size
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(factor) + 0.5), int(h * float(factor) + 0.5)


def _imflip_(img, direction='horizontal'):
    assert direction == 'horizontal'
    img[...] = np.flip(img, 1).copy()
    return img


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, results):
        for t in self.transforms:
            results = t(results)
        return results


FRAMES = {}          # frame_dir -> (total + 1, H, W, 3): entry i is img_{i:05}.jpg


class _SampleFrames:
    """UPSTREAM SampleFrames(clip_len=1, frame_interval=1, num_clips=T), train mode (np.random)."""

    def __call__(self, results):
        results['frame_inds'] = R.sample_frames(results['total_frames'], T, start_index=results['start_index'])
        results['clip_len'], results['frame_interval'], results['num_clips'] = 1, 1, T
        return results


class _RawFrameDecode:
    def __call__(self, results):
        results['imgs'] = [FRAMES[results['frame_dir']][i].copy() for i in results['frame_inds']]
        results['original_shape'] = results['img_shape'] = results['imgs'][0].shape[:2]
        return results


class _MultiScaleCropResize:
    """UPSTREAM MultiScaleCrop(OUT_HW, (1, .875, .75, .66), random_crop=False, max_wh_scale_gap=1, num_fixed_crops=13) + Resize."""

    def __call__(self, results):
        img_h, img_w = results['img_shape']
        x, y, w, h = R.multi_scale_crop_box(img_w, img_h, input_size=(OUT_HW, OUT_HW), num_fixed_crops=13, rng=random)
        results['crop_box'] = (x, y, w, h)
        results['imgs'] = [R.resize_linear_u8(img[y:y + h, x:x + w], OUT_HW, OUT_HW) for img in results['imgs']]
        results['img_shape'] = (OUT_HW, OUT_HW)
        return results


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stubs():
    mmcv = types.ModuleType('mmcv')
    mmcv.imresize = lambda img, size, interpolation='bilinear': R.resize_linear_u8(img, size[0], size[1])
    mmcv.rescale_size = _rescale_size
    mmcv.imflip_ = _imflip_
    mm = types.ModuleType('mmaction')
    ds = types.ModuleType('mmaction.datasets')
    ds.PIPELINES = ds.DATASETS = _NoopRegistry()
    ds.RawframeDataset = type('RawframeDataset', (), {})
    pipes = types.ModuleType('mmaction.datasets.pipelines')
    pipes.Compose = _Compose
    aug = types.ModuleType('mmaction.datasets.pipelines.augmentations')
    aug.Resize, aug.Flip, aug.RandomResizedCrop = _Resize, _Flip, type('RandomResizedCrop', (), {})
    builder = types.ModuleType('mmaction.datasets.builder')
    builder.DATASETS = _NoopRegistry()
    sys.modules.update({'mmcv': mmcv, 'mmaction': mm, 'mmaction.datasets': ds, 'mmaction.datasets.pipelines': pipes,
                        'mmaction.datasets.pipelines.augmentations': aug, 'mmaction.datasets.builder': builder})


def _videos(rng):
    """Five videos: frame sizes (30, 50) and (36, 44); detections in float32 and float64; the cases of the fixture."""
    specs = [  # name, H, W, total, dtype, kind
        ('v_actor_some', 30, 50, 12, np.float32, 'some'),         # boxes in the first half only; overlap; past the edges
        ('v_scene_all', 36, 44, 10, np.float64, 'all'),          # a box in every frame; inverted boxes; score exactly 0.4
        ('v_none', 30, 50, 9, np.float64, 'none'),               # no box above the threshold anywhere
        ('v_mixed', 30, 50, 14, np.float64, 'all'),
        ('v_small', 36, 44, 11, np.float32, 'some'),
    ]
    infos, dets = [], {}
    for label, (name, H, W, total, dt, kind) in enumerate(specs):
        FRAMES[name] = rng.integers(0, 256, (total + 1, H, W, 3)).astype(np.uint8)
        per = []
        for i in range(total + 1):          # entry i is read for frame number i (the 1-based quirk); entry 0 is never read
            rows = []
            if kind == 'none':
                rows = [[3, 4, 20, 25, 0.4], [1, 1, 9, 9, 0.1]]                                  # 0.4 is not > 0.4
            elif kind == 'all' or (kind == 'some' and i <= total // 2):
                x0, y0 = rng.uniform(-5, W - 10), rng.uniform(-5, H - 10)
                rows.append([x0, y0, x0 + rng.uniform(4, 30), y0 + rng.uniform(4, 25), rng.uniform(0.41, 1.0)])
                rows.append([x0 + 2.5, y0 + 3.7, x0 + 12.2, y0 + 9.9, 0.9])                       # overlaps the first
                if i % 3 == 0:
                    rows.append([W - 6.3, H - 7.1, W + 9.0, H + 4.0, 0.8])                       # past the right / bottom edge
                if i % 4 == 1:
                    rows.append([20.7, 15.2, 11.4, 28.6, 0.95])                                  # inverted in x: empty
                rows.append([5.0, 5.0, 25.0, 25.0, 0.4])                                         # exactly at the threshold
            per.append(np.asarray(rows, dtype=dt).reshape(-1, 5))
        dets[name] = per
        infos.append(dict(frame_dir=f'/data/rawframes/{name}', total_frames=total, label=label))
    for v in infos:
        FRAMES[v['frame_dir']] = FRAMES.pop(v['frame_dir'].split('/')[-1])
    return infos, dets


def main():
    _stubs()
    box = _load('ref_box', 'libs/pipelines/box.py')
    acm = _load('ref_acm_loader', 'libs/loader/actor_cut_mix_loader.py')
    ra = _load('ref_rand_augment', 'libs/pipelines/rand_augment.py')
    rng = np.random.default_rng(2024)
    infos, dets = _videos(rng)
    ds = object.__new__(acm.ActorCutMixDataset)
    ds.video_infos = [dict(v, all_detections=dets[v['frame_dir'].split('/')[-1]]) for v in infos]
    ds.filename_tmpl, ds.modality, ds.start_index = 'img_{:05}.jpg', 'RGB', 1

    def chain(last):
        return _Compose([_SampleFrames(), _RawFrameDecode(), box.DetectionLoad(thres=THRES), box.ResizeWithBox(scale=(-1, SHORT)),
                         box.FlipWithBox(flip_ratio=0.5), box.ResizeWithBox(scale=(OUT_HW, OUT_HW), keep_ratio=False)] + last)

    ds.action_pipeline = chain([box.BuildHumanMask(), box.SceneCutOut(fill_color=127)])
    ds.scene_pipeline = chain([box.ActorCutOut(fill_color=127)])
    ds.randAug_pipeline = _Compose([_SampleFrames(), _RawFrameDecode(), _Resize(scale=(-1, SHORT)), ra.RandAugment(n=2, m=10, prob=1),
                                    _MultiScaleCropResize()])
    ds.acm_prob = 0.5
    ds.out_pipeline = _Compose([])
    # every scene pipeline call is recorded (the scene's draws, its int boxes and its painted frames)
    scene_log = []
    orig_scene = ds.scene_pipeline

    def scene_pipeline(results):
        r = orig_scene(results)
        scene_log.append(r)
        return r
    ds.scene_pipeline = scene_pipeline
    randrange_log = []
    orig_randrange = acm.random.randrange

    def randrange(n):
        k = orig_randrange(n)
        randrange_log.append(k)
        return k
    acm.random.randrange = randrange

    out = {'T': np.int64(T), 'short': np.int64(SHORT), 'out_hw': np.int64(OUT_HW), 'thres': np.float64(THRES),
           'n_videos': np.int64(len(infos))}
    for k, v in enumerate(infos):
        name = v['frame_dir'].split('/')[-1]
        out[f'v{k}_frames'] = FRAMES[v['frame_dir']]
        out[f'v{k}_frame_dir'] = np.array(v['frame_dir'])
        out[f'v{k}_total'] = np.int64(v['total_frames'])
        out[f'v{k}_label'] = np.int64(v['label'])
        out[f'v{k}_ndet'] = np.int64(len(dets[name]))
        for i, d in enumerate(dets[name]):
            out[f'v{k}_det{i}'] = d
    # (1) actor_cut_mix on each video as the actor, until every flip combination has been seen
    samples, seen, seed = [], set(), 0
    while len(samples) < 14 or len(seen) < 4:
        random.seed(100 + seed)
        np.random.seed(100 + seed)
        idx = seed % len(infos)
        seed += 1
        res = ds.actor_cut_mix(ds._prepare_frames(idx))
        sc = scene_log[-1]
        seen.add((bool(res['flip']), bool(sc['flip'])))
        samples.append((100 + seed - 1, idx, res, sc, randrange_log[-1]))
    out['n_samples'] = np.int64(len(samples))
    for s, (sd, idx, res, sc, si) in enumerate(samples):
        p = f's{s}_'
        out[p + 'seed'] = np.int64(sd)
        out[p + 'actor'] = np.int64(idx)
        out[p + 'actor_inds'] = np.asarray(res['frame_inds'])
        out[p + 'actor_flip'] = np.int64(res['flip'])
        out[p + 'scene'] = np.int64(si)
        out[p + 'scene_inds'] = np.asarray(sc['frame_inds'])
        out[p + 'scene_flip'] = np.int64(sc['flip'])
        for t in range(T):
            out[p + f'abox{t}'] = res['detections'][t]             # float boxes after the last ResizeWithBox, detection dtype
            out[p + f'sbox{t}'] = sc['detections'][t]
        out[p + 'mask'] = np.stack([m[..., 0] for m in res['human_mask']])
        out[p + 'imgs'] = np.stack(res['imgs'])
        out[p + 'ratio'] = np.float64(res['foreground_ratio'])
        out[p + 'bg_label'] = np.int64(res['background_label'])
    # (2) whole prepare_train_frames calls, acm_prob 0.5: the draws in sample order
    order = [0, 3, 1, 4, 3, 0, 2, 1, 4, 0]
    for seq_seed in range(7, 1000):       # the first seed whose sequence holds both kinds of sample
        random.seed(seq_seed)
        np.random.seed(seq_seed)
        probe = []
        for idx in order:
            state = random.getstate()
            probe.append(random.random() < ds.acm_prob)
            random.setstate(state)
            ds.prepare_train_frames(idx)
        if 0 < sum(probe) < len(probe):
            break
    out['seq_seed'] = np.int64(seq_seed)
    random.seed(seq_seed)
    np.random.seed(seq_seed)
    flags, inds, extra = [], [], []
    for idx in order:
        n_scene = len(scene_log)
        res = ds.prepare_train_frames(idx)
        is_acm = 'human_mask' in res
        flags.append(is_acm)
        inds.append(np.asarray(res['frame_inds']))
        if is_acm:
            sc = scene_log[n_scene]
            extra.append([int(res['flip']), randrange_log[-1], int(sc['flip']), 0, 0])
            out[f'seq{len(flags) - 1}_scene_inds'] = np.asarray(sc['frame_inds'])
        else:
            extra.append([-1] + list(res['crop_box']))
    acm.random.randrange = orig_randrange
    out['seq_order'] = np.asarray(order, np.int64)
    out['seq_acm'] = np.asarray(flags)
    out['seq_inds'] = np.stack(inds)
    out['seq_extra'] = np.asarray(extra, np.int64)       # acm: (actor_flip, scene index, scene_flip, 0, 0); randAug: (-1, x, y, w, h)
    out['seq_next_random'] = np.float64(random.random())
    out['seq_next_np'] = np.float64(np.random.rand())
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes; flip pairs seen', sorted(seen))


if __name__ == '__main__':
    main()
