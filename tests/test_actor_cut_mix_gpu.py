"""ActorCutMix on the GPU: ``bdv_actor_cut_mix_u8`` bit-equal to the numpy restatement of test_actor_cut_mix_cpu.py (over the golden
fixture's clips and edge cases), its host-side validation, ``ActorCutMixClipLoader`` on JPEG files against the CPU chain (Pillow decode,
resize oracle, host boxes, composite, normalize), its other phases against ``RawFrameClipLoader``, ``PrefetchLoader`` around it, and a
two-task ``methods='icarl'`` run with ``accumulate_grad_batches=2``."""
import math
import os
import random

import numpy as np
import pytest
import torch

from oracle import resize_oracle as R
from test_actor_cut_mix_cpu import composite, fixture_videos, flip_resize

pytestmark = pytest.mark.gpu

MEAN = np.array([123.675, 116.28, 103.53], dtype=np.float32)
STD = np.array([58.395, 57.12, 57.375], dtype=np.float32)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'actor_cut_mix_golden.npz')


def _norm(u8):
    """(T, H, W, 3) uint8 -> (T, 3, H, W) fp32 as the kernels normalise: (x - mean) * (1 / std) in fp32."""
    return ((u8.astype(np.float32) - MEAN) * (np.float32(1) / STD)).transpose(0, 3, 1, 2)


def _resized(frames, short):
    out = []
    for f in frames:
        Wr, Hr = R.rescale_size(f.shape[1], f.shape[0], (-1, short))
        out.append(R.resize_linear_u8(f, Wr, Hr))
    return np.stack(out)


def _run_kernel(dev, actor, scene, clips, aboxes, sboxes, B_out, Hd, Wd):
    from bdvcil_amd import kernels as K
    from bdvcil_amd.actor_cut_mix import acm_plan_table
    T = actor.shape[1]
    out = torch.full((B_out, T, 3, Hd, Wd), float('nan'), device=dev)
    table = acm_plan_table(clips, aboxes, sboxes)
    counts = K.actor_cut_mix_u8(torch.from_numpy(actor).to(dev), None if scene is None else torch.from_numpy(scene).to(dev), table,
                                len(clips), out, MEAN.tolist(), STD.tolist())
    return out.cpu().numpy(), counts.cpu().numpy()


def test_kernel_equals_the_restatement_on_the_fixture(dev):
    from bdvcil_amd.actor_cut_mix import clip_boxes
    g = dict(np.load(GOLD))
    infos, dets, frames = fixture_videos(g)
    T, short, S, thres = int(g['T']), int(g['short']), int(g['out_hw']), float(g['thres'])
    n = int(g['n_samples'])
    for s in range(n):       # one launch per clip: the fixture's videos have two sizes
        p = f's{s}_'
        a, sc = infos[int(g[p + 'actor'])], infos[int(g[p + 'scene'])]
        srcs, boxes = [], []
        for v, inds, flip in ((a, g[p + 'actor_inds'], bool(g[p + 'actor_flip'])), (sc, g[p + 'scene_inds'], bool(g[p + 'scene_flip']))):
            fr = frames[v['frame_dir']]
            srcs.append(_resized(fr[inds], short)[None])
            boxes.append(clip_boxes(dets[v['frame_dir'].split('/')[-1]], inds, fr.shape[2], fr.shape[1], short, S, S, flip, thres))
        whole = sum(len(b) for b in boxes[0]) == 0
        clips = [(1, 0, int(g[p + 'actor_flip']), -1 if whole else 0, int(g[p + 'scene_flip']))]
        out, counts = _run_kernel(dev, srcs[0], None if whole else srcs[1], clips, [boxes[0]], [boxes[1]], 3, S, S)
        assert np.array_equal(out[1], _norm(g[p + 'imgs'])), s
        assert np.isnan(out[0]).all() and np.isnan(out[2]).all()          # other rows untouched
        assert counts.tolist() == [int(g[p + 'mask'].astype(np.int64).sum())]
        assert counts[0] / (T * S * S) == float(g[p + 'ratio'])


@pytest.mark.parametrize('Hd,Wd', [(224, 224), (31, 45), (37, 29)])
def test_kernel_edge_cases(Hd, Wd, dev):
    """Hd != Wd, pixel counts not a multiple of 4, boxes touching Wd / Hd, inverted and empty boxes, different actor / scene source
    sizes (incl. the exact-2x and same-size paths), scattered output rows, a clip without boxes next to clips with them."""
    rng = np.random.default_rng(Hd * 100 + Wd)
    T = 3
    actor = rng.integers(0, 256, (4, T, 2 * Hd, 2 * Wd, 3)).astype(np.uint8) if Hd == 224 else \
        rng.integers(0, 256, (4, T, 50, 70, 3)).astype(np.uint8)
    scene = rng.integers(0, 256, (2, T, 41, 57, 3)).astype(np.uint8) if Hd != 224 else rng.integers(0, 256, (2, T, Hd, Wd, 3)).astype(np.uint8)

    def rand_boxes(k):
        out = []
        for t in range(T):
            bs = []
            for _ in range(int(rng.integers(0, 4))):
                x0, x1 = sorted(rng.integers(0, Wd + 1, 2))
                y0, y1 = sorted(rng.integers(0, Hd + 1, 2))
                bs.append([x0, y0, x1, y1])
            if t == k % T:
                bs.append([Wd - 5, Hd - 4, Wd, Hd])                      # touching the right / bottom edge
                bs.append([10, 3, 4, 9])                                  # inverted: empty
            out.append(np.asarray(bs, np.int64).reshape(-1, 4))
        return out
    none = [np.zeros((0, 4), np.int64)] * T
    aboxes = [rand_boxes(0), none, rand_boxes(1), rand_boxes(2)]
    sboxes = [rand_boxes(3), rand_boxes(4), none, rand_boxes(5)]
    clips = [(6, 2, 1, 1, 0), (0, 0, 0, -1, 1), (3, 3, 0, 0, 1), (4, 1, 1, 1, 1)]     # out_row, actor_row, actor_flip, scene_row, scene_flip
    out, counts = _run_kernel(dev, actor, scene, clips, aboxes, sboxes, 7, Hd, Wd)
    for c, (orow, arow, af, srow, sf) in enumerate(clips):
        A = np.stack([R.resize_linear_u8(np.ascontiguousarray(np.flip(f, 1)) if af else f, Wd, Hd) for f in actor[arow]])
        Sc = np.stack([R.resize_linear_u8(np.ascontiguousarray(np.flip(f, 1)) if sf else f, Wd, Hd) for f in scene[max(srow, 0)]])
        img, mask = composite(A, Sc, aboxes[c], sboxes[c])
        assert np.array_equal(out[orow], _norm(img)), c
        assert counts[c] == int(mask.astype(np.int64).sum()), c
    for r in (1, 2, 5):
        assert np.isnan(out[r]).all()


def test_host_validation_refuses_bad_plans(dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError
    from bdvcil_amd.actor_cut_mix import acm_plan_table
    T, S = 2, 16
    actor = torch.zeros(2, T, 20, 20, 3, dtype=torch.uint8, device=dev)
    scene = torch.zeros(1, T, 20, 20, 3, dtype=torch.uint8, device=dev)
    out = torch.full((2, T, 3, S, S), -7.0, device=dev)
    ok = [np.array([[1, 1, 5, 5]])] * T
    bad = [
        ([(0, 0, 0, 0, 0)], [[np.array([[0, 0, S + 1, 4]])] * T], [ok], 'leaves the'),       # box past Wd
        ([(0, 0, 0, 0, 0)], [[np.array([[-1, 0, 3, 4]])] * T], [ok], 'leaves the'),          # negative coordinate
        ([(2, 0, 0, 0, 0)], [ok], [ok], 'output row'),                                       # out_row out of range
        ([(0, 2, 0, 0, 0)], [ok], [ok], 'actor row'),
        ([(0, 0, 0, 1, 0)], [ok], [ok], 'scene row'),                                        # scene row out of range
        ([(0, 0, 0, -1, 0)], [ok], [ok], 'scene row'),                                       # -1 with actor boxes
        ([(0, 0, 2, 0, 0)], [ok], [ok], 'flips'),
    ]
    for clips, ab, sb, msg in bad:
        with pytest.raises(HipExtensionError, match=msg):
            K.actor_cut_mix_u8(actor, scene, acm_plan_table(clips, ab, sb), 1, out, MEAN.tolist(), STD.tolist())
    table = acm_plan_table([(0, 0, 0, 0, 0)], [ok], [ok])
    t2 = table.copy()
    t2[5 + 1] = 7                                                                            # non-monotone offsets
    with pytest.raises(HipExtensionError, match='offsets|boxes'):
        K.actor_cut_mix_u8(actor, scene, t2, 1, out, MEAN.tolist(), STD.tolist())
    with pytest.raises(HipExtensionError, match='plan'):
        K.actor_cut_mix_u8(actor, scene, table[:-1], 1, out, MEAN.tolist(), STD.tolist())
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                                               # nothing was launched


# ---- the loader on files ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def acm_data(tmp_path_factory):
    """Five 'videos' of 10 - 14 JPEG frames (96 x 128, 4:2:0) and a detections.npy with float32 / float64 boxes; video 2 has none."""
    from PIL import Image
    from test_jpeg_cpu import _picture
    root = tmp_path_factory.mktemp('acm_frames')
    rng = np.random.default_rng(31)
    infos, dets = [], {}
    for v in range(5):
        d = root / 'rawframes' / f'v_clip_{v}'
        d.mkdir(parents=True)
        n = 10 + v
        base = _picture(96, 128, v % 3, rng)
        for i in range(1, n + 1):
            Image.fromarray(np.roll(base, (2 * i, 3 * i), axis=(0, 1))).save(str(d / f'img_{i:05}.jpg'), quality=85, subsampling=2)
        dt = np.float32 if v % 2 else np.float64
        per = []
        for i in range(n + 1):
            rows = []
            if v != 2 and (v != 1 or i % 2):
                x0, y0 = rng.uniform(-8, 100), rng.uniform(-8, 70)
                rows = [[x0, y0, x0 + rng.uniform(10, 60), y0 + rng.uniform(10, 50), rng.uniform(0.3, 1.0)], [40, 30, 80, 90, 0.9]]
            per.append(np.asarray(rows, dt).reshape(-1, 5))
        dets[f'v_clip_{v}'] = per
        infos.append({'frame_dir': str(d), 'total_frames': n, 'label': v})
    det_file = root / 'detections.npy'
    np.save(det_file, np.array(dets, dtype=object), allow_pickle=True)
    return infos, str(det_file)


def _pil_clip(info, inds):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(info['frame_dir'], f'img_{int(i):05}.jpg')).convert('RGB')) for i in inds])


def test_train_phase_equals_the_cpu_chain(acm_data, dev):
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader, clip_boxes
    from bdvcil_amd.decode import rescale_size
    infos, det_file = acm_data
    loader = ActorCutMixClipLoader(det_file, acm_prob=0.5, device=dev, short_edge=128, input_size=112, threads=4)
    loader.set_scene_infos(infos)
    batch_infos = [infos[0], infos[2], infos[1], infos[3], infos[4], infos[0]]
    Wr, Hr = rescale_size(128, 96, (-1, 128))
    for seed in range(20):                  # a seed whose plan holds both kinds of row
        random.seed(seed); np.random.seed(seed)
        plan = loader.draw(batch_infos, (Hr, Wr))
        kinds = [r.acm for r in plan.rows]
        if any(kinds) and not all(kinds) and any(r.acm and r.frame_inds is not None for r in plan.rows):
            break
    b = loader.run(plan, batch_infos)
    B, T, S = len(batch_infos), 8, 112
    assert tuple(b['imgs'].shape) == (B, T, 3, S, S) and b['imgs'].dtype == torch.float32
    assert b['label'].dtype == torch.int64 and tuple(b['label'].shape) == (B, 1)
    assert b['foreground_ratio'].dtype == torch.float64 and tuple(b['foreground_ratio'].shape) == (B,)
    assert b['background_label'].dtype == torch.int64 and tuple(b['background_label'].shape) == (B, 1)
    got = b['imgs'].cpu().numpy()
    fr, bl = b['foreground_ratio'].cpu().numpy(), b['background_label'].cpu().numpy()[:, 0]
    rand_rows = [k for k, r in enumerate(plan.rows) if not r.acm]
    for k, r in enumerate(plan.rows):
        if not r.acm:
            continue
        sv = plan.scene_infos[r.scene_index]
        A = flip_resize(_pil_clip(batch_infos[k], r.frame_inds), 128, S, r.flip)
        Sc = flip_resize(_pil_clip(sv, r.scene_inds), 128, S, r.scene_flip)
        ab = clip_boxes(loader.video_detections(batch_infos[k]), r.frame_inds, 128, 96, 128, S, S, r.flip)
        sb = clip_boxes(loader.video_detections(sv), r.scene_inds, 128, 96, 128, S, S, r.scene_flip)
        img, mask = composite(A, Sc, ab, sb)
        assert np.array_equal(got[k], _norm(img)), k
        assert fr[k] == mask.astype(np.int64).sum() / (T * S * S) and bl[k] == sv['label'], k
    # the RandAugment rows, for the same draws, on the CPU: Pillow decode -> Resize(-1, 128) (resize oracle) -> RandAugment
    # (augment oracle) -> MultiScaleCrop + Resize(112) (resize oracle) -> Normalize, no mix
    from oracle import augment_oracle as AO
    for k in rand_rows:
        r = plan.rows[k]
        clip = list(_resized(_pil_clip(batch_infos[k], r.frame_inds), 128))
        if r.randaug is not None:
            ops, flip_sign, init_loc = r.randaug
            for name, minval, maxval in ops:
                val = (float(loader.train_front.randaug.m) / 30) * float(maxval - minval) + minval
                clip = [AO.apply_op(name, f, val, flip_sign, init_loc) for f in clip]
        x, y, w, h = r.crop
        want = np.stack([R.resize_linear_u8(np.ascontiguousarray(f[y:y + h, x:x + w]), S, S) for f in clip])
        assert np.array_equal(got[k], _norm(want)), k
        assert fr[k] == 1.0 and bl[k] == -1
    assert set(np.nonzero(bl == -1)[0].tolist()) == set(rand_rows)
    # video 2 has no box above the threshold: as an actor it is the whole clip (ratio 1) and its scene is not needed
    random.seed(3); np.random.seed(3)
    loader.acm_prob = 1.0
    b2 = loader([infos[2], infos[3]], 'train')
    assert b2['foreground_ratio'][0].item() == 1.0 and b2['foreground_ratio'][1].item() < 1.0
    assert b2['background_label'][0, 0].item() != -1


def test_other_phases_equal_the_rawframe_loader(acm_data, dev):
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    from bdvcil_amd.decode import RawFrameClipLoader
    infos, det_file = acm_data
    acm = ActorCutMixClipLoader(det_file, device=dev, threads=4)
    raw = RawFrameClipLoader(dev, threads=4)
    for phase in ('val', 'features_extraction', 'test'):
        a, r = acm(infos[:3], phase), raw(infos[:3], phase)
        assert set(a) == set(r)
        for k in r:
            if torch.is_tensor(r[k]):
                assert torch.equal(a[k], r[k]), (phase, k)
            else:
                assert a[k] == r[k]


def test_mixed_frame_sizes_are_refused(acm_data, tmp_path, dev):
    from PIL import Image
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    infos, det_file = acm_data
    d = tmp_path / 'v_clip_0'
    d.mkdir()
    for i in range(1, 11):
        Image.fromarray(np.zeros((80, 120, 3), np.uint8)).save(str(d / f'img_{i:05}.jpg'))
    odd = {'frame_dir': str(d), 'total_frames': 10, 'label': 0}
    loader = ActorCutMixClipLoader(det_file, device=dev, threads=2)
    with pytest.raises(ValueError, match='v_clip_0'):
        loader([infos[1], odd], 'train')


def test_prefetch_returns_the_same_batches(acm_data, dev):
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    from bdvcil_amd.decode import PrefetchLoader
    infos, det_file = acm_data
    loader = ActorCutMixClipLoader(det_file, device=dev, threads=2)
    lists = [infos[:2], infos[2:], infos[1:4]]
    loader.set_scene_infos(infos)
    random.seed(4); np.random.seed(4); torch.manual_seed(4)
    want = [loader(l, 'train') for l in lists]
    pre = PrefetchLoader(loader, depth=2)
    loader.set_scene_infos(None)
    calls = []
    orig = loader.set_scene_infos
    loader.set_scene_infos = lambda v: (calls.append(len(v)), orig(v))
    pre.set_scene_infos(infos)                                   # forwarded to the loader with the next batch only
    random.seed(4); np.random.seed(4); torch.manual_seed(4)
    got = list(pre.iterate(lists, 'train'))
    assert loader.scene_infos == infos and calls == [len(infos)]
    for g, w in zip(got, want):
        for k in ('imgs', 'label', 'foreground_ratio', 'background_label', 'frame_inds'):
            assert torch.equal(g[k], w[k]), k


def test_two_task_icarl_run(tmp_path, dev):
    from PIL import Image
    import bdvcil_amd.task_loop as TL
    from bdvcil_amd import cil_step
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    from test_task_loop_gpu import _config, _model_cfg
    model = _model_cfg(2)
    model['cls_head']['loss_cls'] = dict(type='ACMSmoothCE', alpha=4)             # the ActorCutMix configs' head
    model['cls_head']['inc_head_config'] = dict(type='SimpleLinear', out_features=2)
    cfg = _config(tmp_path, task_splits=[[0, 1], [2, 3]], ending_task=1, num_epochs_per_task=2, videos_per_gpu=4, testing_videos_per_gpu=4,
                  methods='icarl', accumulate_grad_batches=2, model=model)
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:60, 0:80]
    dets = {}
    for name in ('train', 'val'):
        for rec in TL.read_ann_file(cfg[f'{name}_ann_file']):
            frame_dir, total, label = rec[0], int(rec[1]), int(rec[2])
            if label > 3:
                continue
            d = tmp_path / 'rawframes' / frame_dir
            d.mkdir(parents=True, exist_ok=True)
            base = np.stack([128 + 90 * np.sin((label + 1) * xx / 9.0), 128 + 90 * np.cos((label % 2 + 1) * yy / 7.0),
                             np.full(xx.shape, 60.0 * label)], -1)
            for i in range(1, total + 1):
                frame = np.clip(np.roll(base, 2 * i, axis=1) + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)
                Image.fromarray(frame).save(str(d / f'img_{i:05}.jpg'), quality=80, subsampling=2)
            dets[frame_dir.split('/')[-1]] = [np.array([[10 + j % 7, 8, 50, 45, 0.9]], np.float32) for j in range(total + 1)]
    det_file = tmp_path / 'detections.npy'
    np.save(det_file, np.array(dets, dtype=object), allow_pickle=True)
    torch.manual_seed(7); random.seed(7); np.random.seed(7)
    loader = ActorCutMixClipLoader(str(det_file), acm_prob=0.5, device=dev, short_edge=128, input_size=112, test_crop=('TenCrop', 128),
                                   threads=4)
    seen = []
    orig = cil_step.icarl_training_step

    def spy(current_model, batch_data, *a, **k):
        if 'foreground_ratio' in batch_data:
            seen.append(batch_data['foreground_ratio'].detach().cpu())
        return orig(current_model, batch_data, *a, **k)
    mp = pytest.MonkeyPatch()
    mp.setattr(cil_step, 'icarl_training_step', spy)
    mp.setattr(TL, 'icarl_training_step', spy, raising=False)
    try:
        loop = TL.CILTaskLoop(cfg, loader, device=dev, seed=0, log=lambda *a: None)
        history = loop.train()
    finally:
        mp.undo()
    assert [h['task'] for h in history] == [0, 1]
    assert seen and any(bool((f < 1).any()) for f in seen)
    assert loader.scene_infos is not None and len(loader.scene_infos) >= 4
    work = tmp_path / 'work'
    for t in range(2):
        assert (work / 'ckpt' / f'ckpt_task_{t}.pt').exists() and (work / 'exemplar' / f'exemplar_task_{t}.txt').exists()
        means = torch.load(work / 'ckpt' / f'exemplar_class_mean_task_{t}.pt', weights_only=True)
        vals = list(means.values()) if isinstance(means, dict) else [means]
        assert vals and all(torch.isfinite(torch.as_tensor(v)).all() for v in vals)
        assert all(math.isfinite(v) and 0.0 <= v <= 100.0 for v in history[t]['cnn'].values)
