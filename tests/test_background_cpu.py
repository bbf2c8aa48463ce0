"""Background extraction, host side (no GPU): the Huffman encoder against Pillow's libjpeg-turbo byte for byte, the quality tables,
``resolve_bg_files`` without extraction, and the background bookkeeping of the task loop (libs/cil/cil.py:146-195, :385-393)."""
import ctypes
import io
import os
import types

import numpy as np
import pytest
from PIL import Image

from bdvcil_amd import background as BG
from bdvcil_amd import task_loop as TL
from bdvcil_amd._lib import lib
from bdvcil_amd.decode import jpeg_entropy_decode, jpeg_parse

SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (23, 31), (31, 23), (240, 320), (256, 341)]
QUALITIES = [25, 50, 75, 95, 100]


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([128 + 100 * np.sin(xx / 7.0), 128 + 100 * np.cos(yy / 5.0), (3 * xx + yy) % 256], -1)
    img = smooth + rng.normal(0, 25, (h, w, 3))
    img[::5] = rng.integers(0, 256, img[::5].shape)          # some rows of pure noise: large AC values, long Huffman codes
    return np.clip(img, 0, 255).astype(np.uint8)


def _pillow_jpeg(img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=q)
    return b.getvalue()


@pytest.mark.parametrize('q', QUALITIES)
@pytest.mark.parametrize('hw', SIZES)
def test_entropy_encode_round_trip(hw, q):
    h, w = hw
    data = _pillow_jpeg(_image(h, w, h * 1000 + w + q), q)
    info, coefs = jpeg_entropy_decode(data)
    assert (info.h[0], info.v[0], info.h[1], info.v[1]) == (2, 2, 1, 1)
    ours = BG.entropy_encode(coefs, w, h, q, threads=1)[0]
    assert ours == data
    cap = lib().bdv_jpeg_encode_bound(w, h)
    assert len(data) <= cap
    buf, n = ctypes.create_string_buffer(cap), ctypes.c_size_t()
    assert lib().bdv_jpeg_entropy_encode(coefs.ctypes.data, w, h, q, buf, cap, ctypes.byref(n)) == 0
    assert buf.raw[:n.value] == data


def test_entropy_encode_batch_threads():
    imgs = [_image(23, 31, s) for s in range(7)]
    files = [_pillow_jpeg(im, 95) for im in imgs]
    coefs = np.stack([jpeg_entropy_decode(f)[1] for f in files])
    assert BG.entropy_encode(coefs, 31, 23, 95, threads=4) == files


def test_entropy_encode_small_buffer_raises():
    data = _pillow_jpeg(_image(16, 16, 1), 95)
    _, coefs = jpeg_entropy_decode(data)
    buf, n = ctypes.create_string_buffer(16), ctypes.c_size_t()
    assert lib().bdv_jpeg_entropy_encode(coefs.ctypes.data, 16, 16, 95, buf, 16, ctypes.byref(n)) != 0
    assert n.value == len(data)


def test_quality_tables_match_pillow():
    img = _image(8, 8, 0)
    for q in range(25, 101):
        ref = jpeg_parse(_pillow_jpeg(img, q))
        ours = BG.encode_info(8, 8, q)
        for c in range(3):
            assert list(ours.qt[c]) == list(ref.qt[c]), (q, c)
        assert ours.coef_count == ref.coef_count and list(ours.coef_offset) == list(ref.coef_offset)
        assert list(ours.blocks_w) == list(ref.blocks_w) and list(ours.blocks_h) == list(ref.blocks_h)


@pytest.mark.parametrize('q', [24, 101, 0])
def test_quality_out_of_range_raises(q):
    with pytest.raises(RuntimeError, match='quality'):
        BG.encode_info(16, 16, q)
    _, coefs = jpeg_entropy_decode(_pillow_jpeg(_image(16, 16, 2), 95))
    with pytest.raises(RuntimeError, match='quality'):
        BG.entropy_encode(coefs, 16, 16, q)


def test_resolve_without_extraction(tmp_path):
    real = tmp_path / 'real_bg'
    real.mkdir()
    link = tmp_path / 'bg_link'
    os.symlink(real, link)
    infos = [dict(frame_dir=str(tmp_path / 'frames' / n), total_frames=3, label=0) for n in ('v_b', 'v_a', 'v_c.avi', 'v_d')]
    for name in ('v_a.jpg', 'v_c.jpg', 'v_b.jpg'):
        (real / name).write_bytes(b'x')
    out = BG.resolve_bg_files(infos, str(link), extract_bg_if_not_found=False)
    # order of video_infos, realpath of bg_dir, the suffix quirk (v_c.avi -> v_c.jpg), missing v_d skipped
    assert out == [str(real / 'v_b.jpg'), str(real / 'v_a.jpg'), str(real / 'v_c.jpg')]
    assert BG.bg_file_for('/x/y/v_e.f.g', real) == real / 'v_e.f.jpg'
    assert BG.resolve_bg_files(infos, str(link), extract_bg_if_not_found=False, bg_image_extension='.png') == []
    # created when missing
    fresh = tmp_path / 'a' / 'b' / 'bg'
    assert BG.resolve_bg_files(infos, str(fresh), extract_bg_if_not_found=False) == [] and fresh.is_dir()
    # map_bg_to_video=False: every file of bg_dir, sorted
    (real / 'z.jpg').write_bytes(b'x')
    (real / 'other.png').write_bytes(b'x')
    assert BG.resolve_bg_files(infos, str(link), map_bg_to_video=False) == sorted(
        str(real / n) for n in ('v_a.jpg', 'v_b.jpg', 'v_c.jpg', 'z.jpg', 'other.png'))


def _records(videos, bgs):
    r = TL.RawframeRecords(None, None)
    r.video_infos = [dict(frame_dir=v, total_frames=8, label=0) for v in videos]
    r.bg_files = list(bgs)
    return r


def test_records_extend_merges_bg_files():
    a, b, c = _records(['a'], ['A']), _records(['b'], ['B']), _records(['c'], ['C', 'A'])
    a.extend([b, c])
    assert [v['frame_dir'] for v in a.video_infos] == ['a', 'b', 'c'] and a.bg_files == ['A', 'B', 'C', 'A']
    d = _records(['d'], ['D'])
    d.merge_bg_files = False
    d.extend(b)
    assert [v['frame_dir'] for v in d.video_infos] == ['d', 'b'] and d.bg_files == ['D']


def _loop_stub(keep_all, cbf_full, bg_dir='/bg'):
    cfg = TL.AttrDict(data_root=None, keep_all_backgrounds=keep_all, cbf_full_bg=cbf_full,
                      data=dict(train=dict(bg_dir=bg_dir) if bg_dir else {}))
    stub = types.SimpleNamespace(config=cfg, exemplar_datasets=[_records(['e1'], ['E1', 'T2']), _records(['e2'], ['E2'])],
                                 train_dataset=_records(['t1', 't2'], ['T1', 'T2', 'E2']),
                                 _all_bg_files=dict.fromkeys(['X0', 'T1', 'E1']))
    stub._bg_config = types.MethodType(TL.CILTaskLoop._bg_config, stub)
    return stub


@pytest.mark.parametrize('keep_all,cbf_full,want', [
    (True, False, ['X0', 'T1', 'E1']),                     # keep_all_backgrounds: every background stored so far (cil.py:153-155)
    (True, True, ['X0', 'T1', 'E1']),
    (False, True, ['T1', 'T2', 'E2', 'E1']),               # cbf_full_bg: train set's | exemplars', first-seen order (:157-160)
    (False, False, []),                                    # neither: no background list -> the random-frame fallback
])
def test_cbf_background_rules(keep_all, cbf_full, want):
    stub = _loop_stub(keep_all, cbf_full)
    cbf = TL.CILTaskLoop.build_cbf_dataset(stub)
    assert [v['frame_dir'] for v in cbf.video_infos] == ['e1', 'e2']
    assert cbf.bg_files == want


def test_cbf_without_bg_dir_unchanged():
    stub = _loop_stub(True, True, bg_dir=None)
    cbf = TL.CILTaskLoop.build_cbf_dataset(stub)
    assert [v['frame_dir'] for v in cbf.video_infos] == ['e1', 'e2']
    assert cbf.bg_files == ['E1', 'T2', 'E2']     # merged as the records carry them; nothing else touches the list
