"""Background extraction on the GPU against its oracles: ``np.median(...).astype(np.uint8)`` for the temporal median, Pillow's
libjpeg-turbo (what cv2.imwrite runs, with the same defaults) for the JPEG forward stage and the whole file, and a two-task
``CILTaskLoop`` run whose config names a ``bg_dir`` that starts out empty."""
import io
import os
import pathlib

import numpy as np
import pytest
import torch
from PIL import Image

from bdvcil_amd import background as BG
from bdvcil_amd.decode import jpeg_entropy_decode

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (23, 31), (31, 23), (240, 320), (256, 341)]
QUALITIES = [25, 50, 75, 95, 100]


def _np_median(stack):
    return np.median(stack, axis=0).astype(np.uint8)


def _stacks(F, h, w, rng):
    shape = (F, h, w, 3)
    out = {'random': rng.integers(0, 256, shape, dtype=np.uint8),
           'equal': np.full(shape, rng.integers(0, 256), dtype=np.uint8),
           'sorted': np.sort(rng.integers(0, 256, shape, dtype=np.uint8), axis=0),
           'reverse': np.sort(rng.integers(0, 256, shape, dtype=np.uint8), axis=0)[::-1].copy(),
           'narrow': rng.integers(100, 104, shape, dtype=np.uint8)}
    if F % 2 == 0:
        for lo, hi in ((15, 16), (127, 128), (0, 255)):      # the two middle values in different nibble buckets
            s = np.empty(shape, dtype=np.uint8)
            s[:F // 2] = lo
            s[F // 2:] = hi
            if F > 2:
                s[0] = rng.integers(0, lo + 1, shape[1:])
                s[-1] = rng.integers(hi, 256, shape[1:])
            out[f'mid{lo}_{hi}'] = s[rng.permutation(F)]
    return out


# every count at the small sizes; the full UCF101 frame size up to the typical video length
MEDIAN_CASES = [(F, hw) for hw in ((1, 1), (7, 9)) for F in (1, 2, 3, 4, 5, 16, 17, 187, 1000)] + \
    [(F, (240, 320)) for F in (1, 2, 3, 4, 5, 16, 17, 187)]


@pytest.mark.parametrize('F,hw', MEDIAN_CASES)
def test_temporal_median(dev, F, hw):
    rng = np.random.default_rng(F * 7 + hw[0])
    for name, stack in _stacks(F, *hw, rng).items():
        got = BG.temporal_median(torch.from_numpy(stack).to(dev), [F]).cpu().numpy()[0]
        np.testing.assert_array_equal(got, _np_median(stack), err_msg=f'{name} F={F} {hw}')


@pytest.mark.parametrize('hw', [(7, 9), (240, 320)])
def test_temporal_median_ragged_batch(dev, hw):
    rng = np.random.default_rng(5)
    counts = [1, 2, 17, 4, 187, 3, 16]
    stacks = [rng.integers(0, 256, (c, *hw, 3), dtype=np.uint8) for c in counts]
    stacks[3][:2], stacks[3][2:] = 127, 128
    got = BG.temporal_median(torch.from_numpy(np.concatenate(stacks)).to(dev), counts).cpu().numpy()
    one = [BG.temporal_median(torch.from_numpy(s).to(dev), [len(s)]).cpu().numpy()[0] for s in stacks]
    for v, s in enumerate(stacks):
        np.testing.assert_array_equal(got[v], _np_median(s))
        np.testing.assert_array_equal(got[v], one[v])


def test_temporal_median_rejects_bad_counts(dev):
    frames = torch.zeros(4, 2, 2, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        BG.temporal_median(frames, [3, 2])
    with pytest.raises(ValueError):
        BG.temporal_median(frames, [4, 0])


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([128 + 100 * np.sin(xx / 7.0), 128 + 100 * np.cos(yy / 5.0), (3 * xx + yy) % 256], -1)
    img = smooth + rng.normal(0, 25, (h, w, 3))
    img[::5] = rng.integers(0, 256, img[::5].shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def _pillow_jpeg(img, q=95):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=q)
    return b.getvalue()


@pytest.mark.parametrize('q', QUALITIES)
@pytest.mark.parametrize('hw', SIZES)
def test_forward_stage_matches_libjpeg(dev, hw, q):
    h, w = hw
    imgs = [_image(h, w, s + q) for s in range(3)]
    imgs[2][:] = imgs[2][:, :1]                     # flat rows: long zero runs
    coefs = BG.jpeg_forward(torch.from_numpy(np.stack(imgs)).to(dev), q).cpu().numpy()
    for k, im in enumerate(imgs):
        _, ref = jpeg_entropy_decode(_pillow_jpeg(im, q))
        np.testing.assert_array_equal(coefs[k], ref, err_msg=f'image {k} {hw} q={q}')


def test_encode_jpeg_mixed_sizes(dev):
    imgs = [_image(h, w, h + w) for h, w in SIZES] + [_image(23, 31, 99)]
    for q in (25, 95, 100):
        assert BG.encode_jpeg(imgs, q) == [_pillow_jpeg(im, q) for im in imgs]
    batch = np.stack([_image(31, 23, s) for s in range(5)])
    assert BG.encode_jpeg(torch.from_numpy(batch).to(dev)) == [_pillow_jpeg(im) for im in batch]


def _write_video(d, F, h, w, seed, q=90):
    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    base = _image(h, w, seed).astype(np.int16)
    for i in range(1, F + 1):
        frame = np.clip(np.roll(base, 3 * i, axis=1) + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        if i % 3 == 0:
            frame[h // 3: h // 2, w // 4: w // 2] = rng.integers(0, 256, 3)       # a moving "foreground" patch
        Image.fromarray(frame).save(str(d / f'img_{i:05}.jpg'), quality=q)


def _pillow_background(d):
    frames = np.stack([np.asarray(Image.open(p).convert('RGB')) for p in sorted(d.glob('*'))])
    med = _np_median(frames)
    return med, _pillow_jpeg(med, 95)


@pytest.mark.parametrize('F,hw', [(1, (24, 40)), (2, (24, 40)), (7, (33, 45)), (187, (240, 320))])
def test_extract_background(dev, tmp_path, F, hw):
    d = tmp_path / 'frames' / 'v_x'
    _write_video(d, F, *hw, seed=F)
    med, data = _pillow_background(d)
    dest = tmp_path / 'bg' / 'v_x.jpg'
    got = BG.extract_background(d, dest)
    np.testing.assert_array_equal(got, med)
    assert dest.read_bytes() == data
    assert [p.name for p in dest.parent.iterdir()] == ['v_x.jpg']          # no temporary file left


def test_resolve_with_extraction(dev, tmp_path):
    frames = tmp_path / 'frames'
    sizes = {'v_a': (24, 40), 'v_b': (33, 45), 'v_c.avi': (24, 40), 'v_d': (24, 40)}
    for i, (n, hw) in enumerate(sizes.items()):
        _write_video(frames / n, 5 + i, *hw, seed=i)
    bg = pathlib.Path(os.path.realpath(tmp_path)) / 'bg'
    bg.mkdir()
    (bg / 'v_b.jpg').write_bytes(b'existing')
    old = os.stat(bg / 'v_b.jpg').st_mtime_ns
    infos = [dict(frame_dir=str(frames / n), total_frames=5, label=0) for n in ('v_d', 'v_b', 'v_a', 'v_c.avi')]
    out = BG.resolve_bg_files(infos, str(bg), max_batch_bytes=40 * 24 * 40 * 3)      # forces several batches
    assert out == [str(bg / n) for n in ('v_d.jpg', 'v_b.jpg', 'v_a.jpg', 'v_c.jpg')]
    assert (bg / 'v_b.jpg').read_bytes() == b'existing' and os.stat(bg / 'v_b.jpg').st_mtime_ns == old
    for n in ('v_a', 'v_c.avi', 'v_d'):
        assert (bg / BG.bg_file_for(n, bg).name).read_bytes() == _pillow_background(frames / n)[1], n
    # a frame directory with frames of two sizes: an error naming it, no file behind
    bad = frames / 'v_bad'
    _write_video(bad, 4, 24, 40, seed=9)
    Image.fromarray(_image(24, 48, 1)).save(str(bad / 'img_00005.jpg'), quality=90)
    with pytest.raises(ValueError, match='v_bad'):
        BG.resolve_bg_files([dict(frame_dir=str(bad), total_frames=5, label=0)], str(bg))
    assert not (bg / 'v_bad.jpg').exists()
    assert sorted(p.name for p in bg.iterdir()) == ['v_a.jpg', 'v_b.jpg', 'v_c.jpg', 'v_d.jpg']


def test_two_tasks_extract_backgrounds(tmp_path):
    """test_rawframe_run_gpu.py's run with ``data.train.bg_dir`` naming an empty directory: every train video gets its background,
    and each fit's loader sees the current task's backgrounds plus the exemplars'."""
    import bdvcil_amd.task_loop as TL
    from bdvcil_amd.decode import RawFrameClipLoader
    from test_task_loop_gpu import _config
    cfg = _config(tmp_path, task_splits=[[0, 1], [2, 3]], ending_task=1, num_epochs_per_task=1, videos_per_gpu=4, testing_videos_per_gpu=4)
    bg_dir = tmp_path / 'bg_extract'
    bg_dir.mkdir()
    cfg['data']['train'] = dict(type='BackgroundMixDataset', bg_dir=str(bg_dir))
    for name in ('train', 'val'):
        for k, rec in enumerate(TL.read_ann_file(cfg[f'{name}_ann_file'])):
            if int(rec[2]) > 3:
                continue
            _write_video(tmp_path / 'rawframes' / rec[0], int(rec[1]), 60, 80, seed=k + (0 if name == 'train' else 500), q=80)

    class Recording(RawFrameClipLoader):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.seen = []

        def set_bg_files(self, bg_files):
            self.seen.append(list(bg_files))
            super().set_bg_files(bg_files)

    loader = Recording('cuda', short_edge=128, input_size=112, bg_resize=128, test_crop=('TenCrop', 128), threads=4)
    loop = TL.CILTaskLoop(cfg, loader, device='cuda', seed=0, log=lambda *a: None)
    history = loop.train()
    assert [h['task'] for h in history] == [0, 1]
    per_task = []
    for t in (0, 1):
        recs = TL.RawframeRecords(str(loop.files.task_splits_ann_files['train'][t]), cfg['data_root'])
        names = [os.path.basename(v['frame_dir']) for v in recs.video_infos]
        assert names and all((bg_dir / f'{n}.jpg').exists() for n in names), t
        per_task.append([str(bg_dir / f'{n}.jpg') for n in names])
    ex0 = TL.RawframeRecords(str(loop.files.exemplar_ann_file(0)), cfg['data_root'])
    ex_bg = [str(bg_dir / (os.path.basename(v['frame_dir']) + '.jpg')) for v in ex0.video_infos]
    real = os.path.realpath
    seen = [[real(p) for p in s] for s in loader.seen]
    assert seen[0] == [real(p) for p in per_task[0]]
    assert seen[1] == [real(p) for p in per_task[1] + ex_bg]
    # one extracted background against Pillow's median + encode
    v0 = TL.RawframeRecords(str(loop.files.task_splits_ann_files['train'][0]), cfg['data_root']).video_infos[0]['frame_dir']
    assert (bg_dir / (os.path.basename(v0) + '.jpg')).read_bytes() == _pillow_background(pathlib.Path(v0))[1]


def test_prefetch_loader_forwards_bg_files(dev):
    from bdvcil_amd.decode import PrefetchLoader

    class Loader:
        def __init__(self):
            self.bg, self.calls = None, []

        def set_bg_files(self, bg_files):
            self.bg = list(bg_files)

        def __call__(self, video_infos, phase):
            self.calls.append((video_infos[0], self.bg))
            return {'imgs': torch.zeros(1, device=dev)}

    inner = Loader()
    pf = PrefetchLoader(inner)
    pf.submit(['a'], 'train')
    pf.set_bg_files(['x.jpg', 'y.jpg'])
    pf.submit(['b'], 'train')
    pf.set_bg_files([])
    pf.submit(['c'], 'train')
    for _ in range(3):
        pf.get()
    assert inner.calls == [('a', None), ('b', ['x.jpg', 'y.jpg']), ('c', [])]
