"""A CIL config run end to end on files: loader-owned random state (a seeded loader returns the batches of the unseeded loader after
seeding the process-global generators), the task loop fed through ``PrefetchLoader`` (same checkpoints, exemplars, class means and
accuracy tables as with the loader called inline; a loader exception surfaces on the training thread and leaves no thread behind),
loaders built from config settings for the two dataset families the hard-coded pipeline got wrong (``no_aug``: nothing is mixed;
plain ``RawframeDataset``: no background at all), and ``tools/train_cil.py`` on a config file.  Toy sizes: 80 x 60 JPEG frames, 20
per video, TSM-R18 at 112 x 112."""
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from test_task_loop_gpu import _config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(short_edge=128, input_size=112, bg_resize=128, test_crop=('TenCrop', 128), threads=4)


def _seed_globals(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """4 classes: class c has 5 - c % 2 train videos (so classes 0, 1 hold 9) and 2 val videos, 20 frames each; 3 backgrounds."""
    from PIL import Image
    root = tmp_path_factory.mktemp('prefetch_data')
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:60, 0:80]
    lines = {'train': [], 'val': []}
    for label in range(4):
        base = np.stack([128 + 90 * np.sin((label + 1) * xx / 9.0), 128 + 90 * np.cos((label % 2 + 1) * yy / 7.0),
                         np.full(xx.shape, 60.0 * label)], -1)
        for name, n in (('train', 5 - label % 2), ('val', 2)):
            for k in range(n):
                rel = f'class{label}/{name}_v{label}_{k}'
                d = root / 'rawframes' / rel
                d.mkdir(parents=True)
                for i in range(1, 21):
                    frame = np.clip(np.roll(base, 2 * i + k, axis=1) + rng.normal(0, 8, base.shape), 0, 255).astype(np.uint8)
                    Image.fromarray(frame).save(str(d / f'img_{i:05}.jpg'), quality=80, subsampling=2)
                lines[name].append(f'{rel} 20 {label}\n')
    for name in lines:
        (root / f'{name}.txt').write_text(''.join(lines[name]))
    (root / 'bg').mkdir()
    bgs = []
    for k in range(3):
        p = root / 'bg' / f'bg_{k}.jpg'
        Image.fromarray(rng.integers(0, 256, (90, 120, 3)).astype(np.uint8)).save(str(p), quality=85)
        bgs.append(str(p))
    infos = [dict(frame_dir=str(root / 'rawframes' / ln.split()[0]), total_frames=20, label=int(ln.split()[2])) for ln in lines['train']]
    return dict(root=root, bgs=bgs, infos=infos)


def _cfg(toy, run_dir, **over):
    kw = dict(task_splits=[[0, 1]], ending_task=0, num_epochs_per_task=2, videos_per_gpu=4, testing_videos_per_gpu=4,
              data_root=str(toy['root'] / 'rawframes'), train_ann_file=str(toy['root'] / 'train.txt'), val_ann_file=str(toy['root'] / 'val.txt'))
    kw.update(over)
    run_dir.mkdir(parents=True, exist_ok=True)
    return _config(run_dir, **kw)


# ---- seeded loader == seeded globals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4, 3])
def test_seeded_loader_equals_seeded_globals(toy, n):
    """Bit-equal batches, with backgrounds from files and with the random-frame fallback (which draws from ``random``, the generator
    RandAugment and MultiScaleCrop use too); 3 and 4 videos; the globals stay untouched by the seeded loader."""
    from bdvcil_amd.decode import RawFrameClipLoader
    infos = toy['infos'][1:1 + n]
    for bgs in (toy['bgs'], None):
        _seed_globals(7)
        want = RawFrameClipLoader('cuda', bg_files=bgs, **SMALL)(infos, 'train')
        _seed_globals(1234)
        state = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state())
        got = RawFrameClipLoader('cuda', bg_files=bgs, seed=7, **SMALL)(infos, 'train')
        assert random.getstate() == state[0] and (np.random.get_state()[1] == state[1]).all() and torch.equal(torch.get_rng_state(), state[2])
        for key in ('imgs', 'randAug', 'frame_inds'):
            assert torch.equal(got[key], want[key]), (key, bgs is None)
        assert tuple(got['imgs'].shape) == (n, 8, 3, 112, 112)
        other = RawFrameClipLoader('cuda', bg_files=bgs, seed=8, **SMALL)(infos, 'train')
        assert not torch.equal(other['imgs'], want['imgs'])


def test_seeded_actor_cut_mix_loader_equals_seeded_globals(toy, tmp_path):
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    rng = np.random.default_rng(5)
    dets = {}
    for v in toy['infos']:
        per = []
        for i in range(21):                       # indexed by the 1-based frame number
            x0, y0 = rng.uniform(0, 40), rng.uniform(0, 25)
            per.append(np.asarray([[x0, y0, x0 + rng.uniform(10, 35), y0 + rng.uniform(10, 30), rng.uniform(0.3, 1.0)]], np.float32))
        dets[v['frame_dir'].split('/')[-1]] = per
    det_file = tmp_path / 'detections.npy'
    np.save(det_file, np.array(dets, dtype=object), allow_pickle=True)
    kw = dict(acm_prob=0.5, short_edge=128, input_size=112, test_crop=('TenCrop', 128), threads=4)
    infos = toy['infos'][:5]
    _seed_globals(7)
    a = ActorCutMixClipLoader(str(det_file), **kw)
    a.set_scene_infos(toy['infos'])
    want = [a(infos, 'train'), a(infos[:3], 'train')]
    _seed_globals(99)
    b = ActorCutMixClipLoader(str(det_file), seed=7, **kw)
    b.set_scene_infos(toy['infos'])
    got = [b(infos, 'train'), b(infos[:3], 'train')]
    kinds = set()
    for g, w in zip(got, want):
        for key in ('imgs', 'frame_inds', 'foreground_ratio', 'background_label'):
            assert torch.equal(g[key], w[key]), key
        kinds |= set((w['background_label'].reshape(-1) >= 0).tolist())
    assert kinds == {True, False}                 # both branches (ActorCutMix and RandAugment rows) were drawn


# ---- the loop through the prefetcher -------------------------------------------------------------------------------------------------
class _Runs:
    """One-task runs of the loop (2 epochs over 9 videos at 4 per batch: 3 batches, the last with 1 clip), per prefetch depth."""

    def __init__(self, toy, base):
        self.toy, self.base, self.done = toy, base, {}

    def get(self, prefetch):
        if prefetch not in self.done:
            import bdvcil_amd.heads
            import bdvcil_amd.task_loop as TL
            from bdvcil_amd.decode import RawFrameClipLoader
            run = self.base / f'prefetch_{prefetch}'
            _seed_globals(11)                        # model initialisation, and the seed the dropout masks are derived from
            bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0    # ... together with this per-process count of the masks drawn so far
            loader = RawFrameClipLoader('cuda', bg_files=self.toy['bgs'], seed=7, **SMALL)
            loop = TL.CILTaskLoop(_cfg(self.toy, run), loader, device='cuda', seed=0, log=lambda *a: None, prefetch=prefetch)
            assert len(loop.train_dataset) == 9
            history = loop.train()
            loop.close()
            tester = TL.CILTaskLoop(_cfg(self.toy, run), loader, device='cuda', seed=0, log=lambda *a: None, prefetch=prefetch)
            tables = tester.cil_testing(test_nme=True)
            tester.close()
            work = run / 'work'
            self.done[prefetch] = dict(
                ckpt=torch.load(work / 'ckpt' / 'ckpt_task_0.pt', map_location='cpu', weights_only=True),
                means=torch.load(work / 'ckpt' / 'exemplar_class_mean_task_0.pt', map_location='cpu', weights_only=True),
                exemplar=(work / 'exemplar' / 'exemplar_task_0.txt').read_text(), tables=tables, loss=history[0]['train_loss'],
                results=((work / 'cnn_result.txt').read_text(), (work / 'nme_result.txt').read_text()))
        return self.done[prefetch]


@pytest.fixture(scope='module')
def runs(toy, tmp_path_factory):
    return _Runs(toy, tmp_path_factory.mktemp('prefetch_runs'))


@pytest.mark.parametrize('depth', [2, 5])
def test_prefetch_on_equals_prefetch_off(runs, depth):
    """``prefetch=5`` is deeper than the epoch (3 batches)."""
    off, on = runs.get(0), runs.get(depth)
    assert off['ckpt'].keys() == on['ckpt'].keys() and len(off['ckpt']) > 50
    for k in off['ckpt']:
        assert torch.equal(off['ckpt'][k], on['ckpt'][k]), k
    assert off['loss'] == on['loss'] and len(off['loss']) == 2 and all(np.isfinite(off['loss']))


def test_predict_and_feature_extraction_through_the_prefetcher(runs):
    off, on = runs.get(0), runs.get(2)
    assert off['exemplar'] == on['exemplar'] and len(off['exemplar'].splitlines()) == 4          # budget 2 per class
    assert torch.equal(off['means']['class_means'], on['means']['class_means']) and torch.isfinite(off['means']['class_means']).all()
    assert off['tables'] == on['tables'] and set(off['tables']) == {'cnn', 'nme'}
    assert off['results'] == on['results']


# ---- the two policies the hard-coded pipeline got wrong ------------------------------------------------------------------------------
def _plain(toy, loader, batch, infos):
    """Crop + resize + normalize of the batch's frames alone: the files decoded and resized here, the loader's crop boxes."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd.decode import JpegDecoder, rescale_size
    from bdvcil_amd.frontend import BackgroundMixFrontEnd, MultiScaleCropResize
    dec = JpegDecoder('cuda', threads=2)
    clips = []
    for v, inds in zip(infos, batch['frame_inds'].tolist()):
        streams = []
        for i in inds:
            with open(os.path.join(v['frame_dir'], f'img_{i:05}.jpg'), 'rb') as f:
                streams.append(f.read())
        clips.append(streams)
    frames = dec.decode_clips(clips)
    Wr, Hr = rescale_size(80, 60, (-1, 256))
    frames = K.resize_linear_u8(frames, Hr, Wr)
    crop = MultiScaleCropResize(input_size=224, num_fixed_crops=13)
    frames, _ = crop(frames, None, boxes=loader.train_front.crop_resize.last_boxes)
    return BackgroundMixFrontEnd().as_nchw(frames, None, None)


@pytest.mark.parametrize('family,seed', [('ucf101/no_aug/seed_1000_inc_10_stages_no_aug.py', 3),
                                         ('ucf101/icarl_video_mix/icarl_seed_1000_inc_10_stages_video_mix.py', 6)])
def test_config_built_loader_mixes_nothing(toy, family, seed):
    from bdvcil_amd.config_run import build_clip_loader, clip_loader_spec
    from bdvcil_amd.decode import RawFrameClipLoader
    with open(os.path.join(ROOT, 'tests', 'golden', 'cil_configs.json')) as f:
        cfg = json.load(f)[family]
    infos = toy['infos'][2:6]
    loader = build_clip_loader(cfg, seed=seed, threads=4)
    loader.set_bg_files(['/no/such/dir/bg_a.jpg', '/no/such/dir/bg_b.jpg'])          # opening one of these would raise
    batch = loader(infos, 'train')
    want = _plain(toy, loader, batch, infos)
    fired = batch['randAug'].cpu()
    if 'no_aug' in family:
        assert not fired.any()
    else:
        assert fired.any() and (~fired).any()      # RandAugment (prob 0.5) on its own: compare the clips it left alone
    keep = (~fired).nonzero().reshape(-1).to('cuda')
    assert torch.equal(batch['imgs'][keep], want[keep])
    # the pipeline every loader used to be: RandAugment decides, and the clips it skipped are mixed with a background
    kw = dict(clip_loader_spec(cfg)['kwargs'])
    for k in ('with_randAug', 'prob', 'bg_mix'):
        kw.pop(k, None)
    old = RawFrameClipLoader('cuda', seed=seed, threads=4, bg_files=toy['bgs'], **kw)(infos, 'train')
    assert torch.equal(old['frame_inds'], batch['frame_inds']) and torch.equal(old['randAug'].cpu(), fired)
    for b in keep.tolist():
        assert not torch.equal(old['imgs'][b], want[b])


# ---- a loader exception on the worker thread -----------------------------------------------------------------------------------------
class _Boom:
    def __init__(self, loader, at):
        self.loader, self.at, self.calls = loader, at, 0

    def __call__(self, infos, phase):
        self.calls += 1
        if self.calls - 1 == self.at:
            raise RuntimeError(f'boom at {self.at}')
        return self.loader(infos, phase)


def test_worker_exception_surfaces_and_releases_the_thread(toy, tmp_path):
    """A Python exception on the host worker thread (no device fault is involved)."""
    import bdvcil_amd.task_loop as TL
    from bdvcil_amd.decode import RawFrameClipLoader
    loader = RawFrameClipLoader('cuda', bg_files=toy['bgs'], seed=7, **SMALL)
    loader(toy['infos'][:4], 'train')                  # the decoder's own pool threads exist from here on
    _seed_globals(11)
    loop = TL.CILTaskLoop(_cfg(toy, tmp_path / 'a'), _Boom(loader, 2), device='cuda', seed=0, log=lambda *a: None, prefetch=2)
    steps, real = [], loop._training_step
    loop._training_step = lambda batch: (steps.append(1), real(batch))[1]
    before = threading.active_count()
    with pytest.raises(RuntimeError) as err:
        loop.fit(loop.train_dataset, 1)
    assert type(err.value) is RuntimeError and str(err.value) == 'boom at 2'
    assert len(steps) == 2
    assert loop._prefetcher.queue == [] and loop._prefetcher.pool is None
    loop.close()
    assert not [t.name for t in threading.enumerate() if t.name.startswith('bdv_prefetch')]
    assert threading.active_count() <= before
    fresh = TL.CILTaskLoop(_cfg(toy, tmp_path / 'b'), loader, device='cuda', seed=0, log=lambda *a: None, prefetch=2)
    losses = fresh.fit(fresh.train_dataset, 1)
    fresh.close()
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert not [t.name for t in threading.enumerate() if t.name.startswith('bdv_prefetch')]


# ---- the command ---------------------------------------------------------------------------------------------------------------------
def test_train_cil_command(toy, tmp_path):
    base = _cfg(toy, tmp_path / 'run', task_splits=[[0, 1], [2, 3]], ending_task=1, num_epochs_per_task=1)
    lines = ['import os', "data_dir = os.environ['VIDEO_CIL_ROOT']"]
    for k, v in base.items():
        if k not in ('data', 'data_root', 'train_ann_file', 'val_ann_file'):
            lines.append(f'{k} = {v!r}')
    lines.append('''
data_root = os.path.join(data_dir, 'rawframes')
train_ann_file = os.path.join(data_dir, 'train.txt')
val_ann_file = os.path.join(data_dir, 'val.txt')
randAug_prob = 0.75
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_bgr=False)
def _eval(crop):
    return [dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8, test_mode=True), dict(type='RawFrameDecode'),
            dict(type='Resize', scale=(-1, 128)), crop, dict(type='Normalize', **img_norm_cfg),
            dict(type='FormatShape', input_format='NCHW'), dict(type='Collect', keys=['imgs', 'label'], meta_keys=[]),
            dict(type='ToTensor', keys=['imgs'])]
train_pipeline = [
    dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8), dict(type='RawFrameDecode'),
    dict(type='Resize', scale=(-1, 128)), dict(type='RandAugment', n=2, m=10, prob=randAug_prob),
    dict(type='MultiScaleCrop', input_size=112, scales=(1, 0.875, 0.75, 0.66), random_crop=False, max_wh_scale_gap=1, num_fixed_crops=13),
    dict(type='Resize', scale=(112, 112), keep_ratio=False), dict(type='Normalize', **img_norm_cfg),
    dict(type='FormatShape', input_format='NCHW'), dict(type='Collect', keys=['imgs', 'label', 'randAug'], meta_keys=[]),
    dict(type='ToTensor', keys=['imgs', 'label'])]
dataset_type = 'BackgroundMixDataset'
data = dict(
    train=dict(type=dataset_type, ann_file='', bg_dir=os.path.join(data_dir, 'bg'), data_prefix=data_root, pipeline=train_pipeline, alpha=0.5,
               with_randAug=True, bg_resize=128, bg_crop_size=(112, 112), extract_bg_if_not_found=False, map_bg_to_video=False,
               merge_bg_files=False),
    val=dict(type=dataset_type, ann_file='', pipeline=_eval(dict(type='CenterCrop', crop_size=112)), test_mode=True),
    test=dict(type=dataset_type, ann_file='', pipeline=_eval(dict(type='TenCrop', crop_size=128)), test_mode=True),
    features_extraction=dict(type=dataset_type, ann_file='', pipeline=_eval(dict(type='CenterCrop', crop_size=112)), test_mode=True),
    features_extraction_epochs=1)
''')
    path = tmp_path / 'toy_cil_config.py'
    path.write_text('\n'.join(lines))
    env = dict(os.environ, VIDEO_CIL_ROOT=str(toy['root']))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train_cil.py'), str(path), '--seed', '3', '--threads', '4']
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    work = tmp_path / 'run' / 'work'
    assert (work / 'ckpt' / 'ckpt_task_1.pt').exists() and (work / 'exemplar' / 'exemplar_task_1.txt').exists()
    first = (work / 'cnn_result.txt').read_text()
    assert 'task 1' in first and 'task 1' in out.stdout
    os.remove(work / 'cnn_result.txt')
    out = subprocess.run(cmd + ['--test', '--prefetch', '0'], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    assert (work / 'cnn_result.txt').read_text() == first and 'task 1' in out.stdout         # rewritten, and the same at any prefetch
