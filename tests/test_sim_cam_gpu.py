"""Simulated-camera-motion backgrounds on the GPU against their oracles: ``torch.nn.functional.interpolate`` on the CPU (what
torchvision's ``resized_crop`` calls) for the resized crop, ``np.nanmedian`` / ``np.nanmean`` + ``.astype(np.uint8)`` for the
NaN-aware reduce, and the whole chain (Pillow decode, torch crop, numpy reduce) for ``extract_backgrounds(method='sim_cam')``."""
import functools
import io
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn
from PIL import Image

import bdvcil_amd as bd
from bdvcil_amd import background as BG

pytestmark = pytest.mark.gpu

# ---- resized crop -----------------------------------------------------------------------------------------------------------------
BOXES7 = [(0, 0, 24, 32), (2, 3, 17, 22), (0, 5, 9, 11), (10, 1, 14, 30), (3, 3, 6, 7), (0, 0, 5, 32), (19, 0, 5, 9)]
CROP_CASES = {                      # name -> (F, H, W, boxes, size, fewest exact zeros torch leaves)
    'seven': (7, 24, 32, BOXES7, (10, 10), 300),
    'one_pixel': (1, 24, 32, [(9, 20, 1, 1)], (10, 10), 0),
    'non_square': (7, 24, 32, BOXES7, (33, 10), 300),
    'ucf': (3, 240, 320, [(0, 0, 240, 320), (100, 200, 68, 90), (20, 100, 200, 150)], (100, 100), 200),
}
CROP_TOL = 1e-3                     # of a grey level: at most 8 + 8 taps, 255 * 16 * 2^-23 = 4.9e-4, doubled


@functools.lru_cache(maxsize=None)
def _crop_frames(F, H, W):
    """Random frames with black bars (rows 0-3 and the last 3) and one black patch in frame 0."""
    x = np.random.default_rng(F * 1000 + H).integers(1, 256, (F, H, W, 3), dtype=np.uint8)
    x[:, :4] = 0
    x[:, -3:] = 0
    x[0, H // 3: H // 3 + 6, W // 4: W // 4 + 10] = 0
    x.setflags(write=False)
    return x


def _torch_resized_crop(frames, boxes, size, antialias):
    """torchvision ``resized_crop`` of the float CHW image (``read_image(...).float()``): crop, then ``interpolate``."""
    out = []
    for fr, (t, l, h, w) in zip(frames, boxes):
        chw = torch.from_numpy(np.ascontiguousarray(fr)).permute(2, 0, 1).float()[:, t:t + h, l:l + w].contiguous()
        r = Fn.interpolate(chw[None], size=size, mode='bilinear', align_corners=False, antialias=antialias)[0]
        out.append(r.permute(1, 2, 0).numpy())
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _crop_reference(name, antialias):
    F, H, W, boxes, size, _ = CROP_CASES[name]
    ref = _torch_resized_crop(_crop_frames(F, H, W), boxes, size, antialias)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize('antialias', [False, True])
@pytest.mark.parametrize('name', list(CROP_CASES))
def test_resized_crop_matches_torch(dev, name, antialias):
    F, H, W, boxes, size, min_zeros = CROP_CASES[name]
    ref = _crop_reference(name, antialias)
    got = BG.resized_crop(torch.from_numpy(_crop_frames(F, H, W).copy()).to(dev), boxes, size, antialias)
    assert got.dtype == torch.float32 and tuple(got.shape) == (F, size[0], size[1], 3) and got.is_cuda
    got = got.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f'{name} antialias={antialias}: max error {err:.3g}, exact zeros torch {(ref == 0).sum()} / here {(got == 0).sum()}')
    assert (ref >= 0).all() and (ref == 0).sum() >= min_zeros          # the inputs do exercise the zero rule
    assert err <= CROP_TOL
    np.testing.assert_array_equal(got == 0, ref == 0)                   # exact zeros where torch has them, and nowhere else


def test_resized_crop_takes_host_frames_and_int_size(dev):
    frames = _crop_frames(7, 24, 32)
    a = BG.resized_crop(frames.copy(), np.asarray(BOXES7), 10).cpu().numpy()
    np.testing.assert_array_equal(a, BG.resized_crop(torch.from_numpy(frames.copy()).to(dev), BOXES7, (10, 10), False).cpu().numpy())
    with pytest.raises(ValueError, match='leaves'):
        BG.resized_crop(frames.copy(), [(0, 0, 25, 32)] * 7, 10)


# ---- NaN-aware reduce -------------------------------------------------------------------------------------------------------------
def _np_reduce(stack, avg_method, zero_is_missing=True):
    x = np.array(stack, dtype=np.float32)
    if zero_is_missing:
        x[x == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)         # all-NaN positions
        r = (np.nanmedian if avg_method == 'median' else np.nanmean)(x, axis=0)
    assert r.dtype == np.float32
    return np.where(np.isnan(r), np.float32(0), r).astype(np.uint8)      # the 0 numpy's cast leaves for NaN on x86


def _stack(F, shape, seed):
    """Floats in [0, 255.5): position 0 missing in every frame, position 1 present in one frame only, a random 30 % of the rest
    missing (NaN or 0, so the present counts take both parities), every fourth position quantised to halves (ties)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 255.5, (F,) + shape).astype(np.float32)
    flat = x.reshape(F, -1)
    flat[:, 3::4] = np.minimum(np.round(flat[:, 3::4] * 2) / 2, 255)
    flat[:, 7::8] = np.minimum(np.round(flat[:, 7::8] / 16) * 16, 240)  # few distinct values: long runs of equal keys
    miss = rng.random(flat.shape) < 0.3
    flat[miss] = np.where(rng.random(int(miss.sum())) < 0.5, np.float32(np.nan), np.float32(0))
    flat[:, 0] = np.where(np.arange(F) % 2 == 0, np.float32(np.nan), np.float32(0))
    flat[:, 1] = np.nan
    flat[F // 2, 1] = 77.75
    assert not (x >= 255.5).any()
    return x


REDUCE_F = [1, 2, 3, 4, 5, 16, 17, 33, 300]
REDUCE_SHAPES = [(5, 7, 3), (10, 10, 3)]


@pytest.mark.parametrize('shape', REDUCE_SHAPES)
@pytest.mark.parametrize('F', REDUCE_F)
def test_nanreduce_matches_numpy(dev, F, shape):
    stack = _stack(F, shape, F * 31 + shape[0])
    present = (~np.isnan(stack) & (stack != 0)).sum(0).reshape(-1)
    assert present[0] == 0 and present[1] == 1
    if F >= 16:
        assert ((present % 2) != (F % 2)).any() and ((present % 2) == (F % 2)).any()
    dstack = torch.from_numpy(stack).to(dev)
    for avg in ('median', 'mean'):
        for zm in (True, False):
            got = BG.temporal_nanreduce(dstack, [F], avg, zero_is_missing=zm)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + shape
            np.testing.assert_array_equal(got.cpu().numpy()[0], _np_reduce(stack, avg, zm), err_msg=f'{avg} zero_is_missing={zm} F={F}')
    assert BG.temporal_nanreduce(dstack, [F]).cpu().numpy().reshape(-1)[0] == 0


@pytest.mark.parametrize('F', [2, 4, 16, 17, 300])
def test_nanreduce_needs_every_key_bit(dev, F):
    """Values that differ only in their lowest mantissa bits: ``base + k * ulp`` for a permutation k of 0..F-1, per position its
    own base (exponents 2^-3 .. 2^7) and its own permutation."""
    rng = np.random.default_rng(F)
    P = 105
    base = rng.uniform(0.125, 255.0, P).astype(np.float32)
    base[::5] = np.float32(255.0) - base[::5] / 1024                     # a run that crosses no power of two
    bits = base.view(np.int32)[None, :] + np.stack([rng.permutation(F) for _ in range(P)], 1).astype(np.int32)
    stack = bits.view(np.float32).copy()
    stack[rng.random(stack.shape) < 0.2] = np.nan
    dstack = torch.from_numpy(stack).to(dev)
    for avg in ('median', 'mean'):
        np.testing.assert_array_equal(BG.temporal_nanreduce(dstack, [F], avg).cpu().numpy()[0], _np_reduce(stack, avg), err_msg=f'{avg} F={F}')


def test_nanreduce_selects_the_exact_float(dev):
    """uint8 truncation hides single-ulp differences, so pin the selected order statistic itself: stacks whose values straddle an
    integer by ulps (``k - 2 ulp .. k + 2 ulp``) truncate to k - 1 or k depending on exactly which float is the median."""
    rng = np.random.default_rng(3)
    P = 96
    k = rng.integers(2, 250, P).astype(np.float32)
    for F in (3, 4, 5, 6, 31, 32):
        offs = np.stack([rng.integers(-F, F + 1, F) for _ in range(P)], 1).astype(np.int32)
        stack = (k.view(np.int32)[None, :] + offs).view(np.float32).copy()
        assert (stack < k[None]).any() and (stack >= k[None]).any()
        want = _np_reduce(stack, 'median')
        assert len(np.unique(want.astype(np.int32) - k.astype(np.int32))) == 2      # both k - 1 and k occur
        got = BG.temporal_nanreduce(torch.from_numpy(stack).to(dev), [F], 'median').cpu().numpy()[0]
        np.testing.assert_array_equal(got, want, err_msg=f'F={F}')


def test_nanreduce_ragged_batch(dev):
    counts = [1, 4, 9, 2]
    stacks = [_stack(c, (5, 7, 3), 100 + c) for c in counts]
    frames = torch.from_numpy(np.concatenate(stacks)).to(dev)
    for avg in ('median', 'mean'):
        got = BG.temporal_nanreduce(frames, counts, avg).cpu().numpy()
        assert got.shape == (4, 5, 7, 3)
        for v, s in enumerate(stacks):
            np.testing.assert_array_equal(got[v], _np_reduce(s, avg), err_msg=f'{avg} video {v}')


def test_nanreduce_saturates(dev):
    stack = np.array([[300.0, -5.0, 255.9, np.inf, -np.inf, 1e9, 254.999, 0.999]], dtype=np.float32)
    for avg in ('median', 'mean'):
        got = BG.temporal_nanreduce(torch.from_numpy(stack).to(dev), [1], avg).cpu().numpy()[0]
        np.testing.assert_array_equal(got, [255, 0, 255, 255, 0, 255, 254, 0])


def test_nanreduce_rejects_bad_counts(dev):
    frames = torch.zeros(4, 2, 2, 3, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        BG.temporal_nanreduce(frames, [3, 2])
    with pytest.raises(ValueError):
        BG.temporal_nanreduce(frames, [4, 0])
    with pytest.raises(ValueError):
        BG.temporal_nanreduce(frames, [])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E_H, E2E_W, E2E_FILES, E2E_SEED = 48, 64, {'v_long': 14, 'v_short': 8}, 21


@pytest.fixture(scope='module')
def videos(tmp_path_factory):
    """Two frame directories of different lengths: 48 x 64 noise with a black bar on top and one on the left, both one MCU (16
    pixels) wide so that the JPEG round trip leaves exact zeros inside them."""
    root = tmp_path_factory.mktemp('sim_cam_frames')
    rng = np.random.default_rng(8)
    for name, n in E2E_FILES.items():
        (root / name).mkdir()
        for i in range(1, n + 1):
            frame = rng.integers(0, 256, (E2E_H, E2E_W, 3), dtype=np.uint8)
            frame[:16] = 0
            frame[:, :16] = 0
            Image.fromarray(frame).save(str(root / name / f'img_{i:05}.jpg'), quality=90)
    return root


def _selected(d, interval):
    return sorted(d.glob('*'))[:-1:interval]


def _cpu_chain(d, boxes, interval, avg_method):
    """Pillow decode, torch crop + resize, zeros -> NaN, numpy reduce: the float image and the crops' zero mask."""
    frames = np.stack([np.asarray(Image.open(p).convert('RGB')) for p in _selected(d, interval)])
    crops = _torch_resized_crop(frames, boxes, (100, 100), False)
    zero = crops == 0
    crops[zero] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = (np.nanmedian if avg_method == 'median' else np.nanmean)(crops, axis=0)
    return np.where(np.isnan(r), np.float32(0), r), zero


@pytest.mark.parametrize('interval', [1, 2])
@pytest.mark.parametrize('avg_method', ['median', 'mean'])
def test_extract_sim_cam(dev, videos, tmp_path, avg_method, interval):
    names = list(E2E_FILES)
    jobs = [(str(videos / n), str(tmp_path / 'bg' / f'{n}.jpg')) for n in names]
    kw = dict(method='sim_cam', avg_method=avg_method, interval=interval)
    got = BG.extract_backgrounds(jobs, return_arrays=True, draws=E2E_SEED, **kw)
    files = [open(dest, 'rb').read() for _, dest in jobs]
    assert sorted(p.name for p in (tmp_path / 'bg').iterdir()) == sorted(f'{n}.jpg' for n in names)     # no temporary file left

    # the same seeded boxes, video by video in job order
    draws = bd.Draws(E2E_SEED)
    decoder = bd.JpegDecoder(dev)
    n_exception = n_total = 0
    for k, n in enumerate(names):
        sel = _selected(videos / n, interval)
        assert [p for p in sel] == BG.sim_cam_frame_files(videos / n, interval)
        boxes = BG.random_resized_crop_boxes(len(sel), E2E_H, E2E_W, draws=draws)
        decoded = decoder.decode([p.read_bytes() for p in sel])
        crops = BG.resized_crop(decoded, boxes, 100, False)
        staged = BG.temporal_nanreduce(crops, [len(sel)], avg_method)
        assert files[k] == BG.encode_jpeg(staged)[0], n
        np.testing.assert_array_equal(got[k], staged.cpu().numpy()[0])
        assert got[k].shape == (100, 100, 3) and got[k].dtype == np.uint8

        ref, zero = _cpu_chain(videos / n, boxes, interval, avg_method)
        # exact zeros inside the bars: torch leaves them, the kernel leaves the same ones, so they are missing on both sides
        assert zero.sum() > 1000
        np.testing.assert_array_equal(crops.cpu().numpy() == 0, zero)
        covered = zero.all(0)                                        # black in every selected frame's crop: exactly 0, no exception
        near = (np.abs(ref - np.round(ref)) <= CROP_TOL) & ~covered  # a crop error of 1e-3 can move these across an integer
        n_exception += int(near.sum())
        n_total += near.size
        want = ref.astype(np.uint8)
        np.testing.assert_array_equal(got[k][~near], want[~near], err_msg=n)
        assert np.abs(got[k].astype(np.int32) - want.astype(np.int32))[near].max(initial=0) <= 1
        assert (got[k][covered] == 0).all()
    assert n_exception < 0.02 * n_total, (n_exception, n_total)       # a property of the CPU chain alone

    # a second run with the same seed writes the same bytes; another seed draws other boxes
    again = [(d, str(tmp_path / 'bg2' / f'{n}.jpg')) for (d, _), n in zip(jobs, names)]
    BG.extract_backgrounds(again, draws=E2E_SEED, **kw)
    assert [open(dest, 'rb').read() for _, dest in again] == files
    one = BG.extract_background(jobs[0][0], tmp_path / 'bg3' / 'one.jpg', draws=E2E_SEED, **kw)
    np.testing.assert_array_equal(one, got[0])
    assert (tmp_path / 'bg3' / 'one.jpg').read_bytes() == files[0]


def test_extract_sim_cam_batches_and_antialias(dev, videos, tmp_path):
    """A budget that forces one batch per video changes nothing (boxes are drawn in job order either way); ``antialias`` and ``size``
    reach the crop kernel."""
    names = list(E2E_FILES)
    jobs = [(str(videos / n), str(tmp_path / 'a' / f'{n}.jpg')) for n in names]
    a = BG.extract_backgrounds(jobs, return_arrays=True, method='sim_cam', draws=3)
    b = BG.extract_backgrounds([(d, str(tmp_path / 'b' / f'{n}.jpg')) for (d, _), n in zip(jobs, names)], return_arrays=True, method='sim_cam',
                               draws=3, max_batch_bytes=1)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    c = BG.extract_background(jobs[0][0], tmp_path / 'c.jpg', method='sim_cam', draws=3, antialias=True, size=(40, 56))
    sel = BG.sim_cam_frame_files(jobs[0][0])
    boxes = BG.random_resized_crop_boxes(len(sel), E2E_H, E2E_W, draws=3)
    crops = BG.resized_crop(bd.JpegDecoder(dev).decode([p.read_bytes() for p in sel]), boxes, (40, 56), True)
    np.testing.assert_array_equal(c, BG.temporal_nanreduce(crops, [len(sel)]).cpu().numpy()[0])
    assert c.shape == (40, 56, 3)
    with Image.open(tmp_path / 'c.jpg') as im:
        assert im.size == (56, 40)


def test_tmf_through_the_new_signature(dev, videos, tmp_path):
    """``method='tmf'`` with every new keyword at its default writes what it wrote before: Pillow's median and encode."""
    d = videos / 'v_short'
    frames = np.stack([np.asarray(Image.open(p).convert('RGB')) for p in sorted(d.glob('*'))])
    med = np.median(frames, axis=0).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(med).save(buf, 'JPEG', quality=95)
    got = BG.extract_backgrounds([(str(d), str(tmp_path / 'tmf.jpg'))], return_arrays=True, method='tmf', avg_method='median', interval=1,
                                 max_frames=500, size=100, antialias=False, draws=None)[0]
    np.testing.assert_array_equal(got, med)
    assert (tmp_path / 'tmf.jpg').read_bytes() == buf.getvalue()
    np.testing.assert_array_equal(BG.extract_background(d, tmp_path / 'tmf2.jpg', method='tmf'), med)
    assert (tmp_path / 'tmf2.jpg').read_bytes() == buf.getvalue()
