"""Host side of the simulated-camera-motion background extraction (``sim_cam_motion_bg_extract``): frame selection, the
``RandomResizedCrop.get_params`` box draws, the two entry points in header / binding / library, argument errors, the CLI parser."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import bdvcil_amd as bd
from bdvcil_amd import background as BG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bdv_resized_crop_f32', 'bdv_temporal_nanreduce_f32')


def _dir_with(tmp_path, n):
    d = tmp_path / f'v_{n}'
    d.mkdir()
    for i in range(1, n + 1):
        (d / f'img_{i:05}.jpg').write_bytes(b'x')
    return d


def test_frame_files(tmp_path):
    d = _dir_with(tmp_path, 10)
    names = lambda files: [int(p.name[4:9]) - 1 for p in files]
    assert names(BG.sim_cam_frame_files(d)) == list(range(9))                 # the last file is always left out
    assert names(BG.sim_cam_frame_files(d, interval=3)) == [0, 3, 6]
    assert names(BG.sim_cam_frame_files(d, max_frames=2)) == [0, 1]
    assert names(BG.sim_cam_frame_files(d, interval=2, max_frames=3)) == [0, 2, 4]
    one = _dir_with(tmp_path, 1)
    with pytest.raises(ValueError, match='v_1'):
        BG.sim_cam_frame_files(one)
    with pytest.raises(FileNotFoundError):
        BG.sim_cam_frame_files(tmp_path / 'missing')
    with pytest.raises(ValueError):
        BG.sim_cam_frame_files(d, interval=0)


def test_boxes_lie_inside_and_reproduce():
    for (h, w) in ((240, 320), (48, 64), (7, 9), (1, 1), (10, 400), (400, 10)):
        b = BG.random_resized_crop_boxes(50, h, w, draws=11)
        assert b.shape == (50, 4) and b.dtype == np.int32
        assert (b[:, :2] >= 0).all() and (b[:, 2:] >= 1).all()
        assert (b[:, 0] + b[:, 2] <= h).all() and (b[:, 1] + b[:, 3] <= w).all()
        np.testing.assert_array_equal(b, BG.random_resized_crop_boxes(50, h, w, draws=11))
        np.testing.assert_array_equal(b, BG.random_resized_crop_boxes(50, h, w, draws=bd.Draws(11)))
    assert not np.array_equal(BG.random_resized_crop_boxes(50, 240, 320, draws=11), BG.random_resized_crop_boxes(50, 240, 320, draws=12))
    # one frame after the other on one generator: 5 + 5 boxes from one bundle are the 10 of a fresh one
    d = bd.Draws(4)
    two = np.concatenate([BG.random_resized_crop_boxes(5, 240, 320, draws=d), BG.random_resized_crop_boxes(5, 240, 320, draws=d)])
    np.testing.assert_array_equal(two, BG.random_resized_crop_boxes(10, 240, 320, draws=4))


def _first_box_by_hand(H, W):
    """The documented order on torch's global generator: area fraction, log aspect ratio, then top, then left."""
    log_ratio = torch.log(torch.tensor([3.0 / 4.0, 4.0 / 3.0]))
    for _ in range(10):
        target_area = H * W * torch.empty(1).uniform_(0.08, 1.0).item()
        aspect = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]))).item()
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            top = int(torch.randint(0, H - h + 1, (1,)).item())
            left = int(torch.randint(0, W - w + 1, (1,)).item())
            return top, left, h, w
    raise AssertionError('no attempt fitted')


@pytest.mark.parametrize('seed', [0, 1, 7])
def test_first_box_on_the_global_generator(seed):
    torch.manual_seed(seed)
    want = _first_box_by_hand(240, 320)
    torch.manual_seed(seed)
    got = BG.random_resized_crop_boxes(1, 240, 320)
    assert tuple(int(x) for x in got[0]) == want
    # a seeded bundle is the stream torch.manual_seed starts
    assert tuple(int(x) for x in BG.random_resized_crop_boxes(1, 240, 320, draws=seed)[0]) == want


def test_fallback_box_and_its_draw_count():
    # 10 x 400: every attempt has h >= sqrt(0.08 * 4000 / (4 / 3)) = 15.5 > 10, so all ten fail: 20 uniform draws, then the
    # fallback without a draw -- in_ratio 40 > 4/3: h = 10, w = round(10 * 4/3) = 13, centred
    assert math.sqrt(0.08 * 4000 / (4.0 / 3.0)) > 10.5
    torch.manual_seed(5)
    got = BG.random_resized_crop_boxes(1, 10, 400)
    after = torch.rand(1).item()
    assert tuple(int(x) for x in got[0]) == (0, 193, 10, 13)
    torch.manual_seed(5)
    log_ratio = torch.log(torch.tensor([3.0 / 4.0, 4.0 / 3.0]))
    for _ in range(10):
        torch.empty(1).uniform_(0.08, 1.0)
        torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]))
    assert torch.rand(1).item() == after
    assert tuple(int(x) for x in BG.random_resized_crop_boxes(1, 400, 10, draws=5)[0]) == (193, 0, 13, 10)
    # an in-range aspect ratio that still cannot fit is impossible (scale <= 1), so the whole-frame branch is reached only
    # through ``scale``: areas above the frame's
    assert tuple(int(x) for x in BG.random_resized_crop_boxes(1, 30, 40, scale=(4.0, 5.0), draws=1)[0]) == (0, 0, 30, 40)


def _header_params(hdr, name):
    m = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\((.*?)\);', hdr, re.S | re.M)
    assert m, f'{name} is not declared in include/bdvcil_hip.h'
    return [p.strip() for p in m.group(1).split(',')]


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    for name in NEW:
        params = _header_params(hdr, name)
        assert hasattr(lib, name), f'{name} is not exported by the built library'
        assert name in bd._lib.SIGNATURES, f'{name} has no ctypes signature'
        res, args = bd._lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert len(args) == len(params), (name, len(args), params)
        for p, a in zip(params, args):       # pointers against pointers, scalars against scalars
            assert ('*' in p) == (a is bd._lib.P), (name, p, a)
    assert 'sim_cam.hip' in bd._lib.HASHED_SOURCES
    assert bd._lib.lib().bdv_abi_version() == bd._lib.ABI_VERSION


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = bd._lib.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the calls fail on their arguments
    box = (ctypes.c_int32 * 4)(0, 0, 5, 9)
    host = ctypes.cast(box, ctypes.c_void_p)
    assert lib.bdv_resized_crop_f32(one, 1, 4, 8, one, host, 10, 10, 0, one, None) == -1 and b'leaves' in lib.bdv_last_error()
    assert lib.bdv_resized_crop_f32(one, 1, 4, 8, one, None, 10, 10, 0, one, None) == -1 and b'null' in lib.bdv_last_error()
    box[2], box[3] = 4, 8
    assert lib.bdv_resized_crop_f32(one, 1, 4, 8, one, host, 10, 10, 2, one, None) == -1 and b'antialias' in lib.bdv_last_error()
    assert lib.bdv_resized_crop_f32(one, 1, 4, 8, one, host, 0, 10, 0, one, None) == -1 and b'sizes' in lib.bdv_last_error()
    first, counts = (ctypes.c_int64 * 2)(0, 3), (ctypes.c_int32 * 2)(3, 2)
    fh, ch = ctypes.cast(first, ctypes.c_void_p), ctypes.cast(counts, ctypes.c_void_p)
    assert lib.bdv_temporal_nanreduce_f32(one, 4, one, one, fh, ch, 2, 12, 0, 1, one, None) == -1 and b'video 1' in lib.bdv_last_error()
    assert lib.bdv_temporal_nanreduce_f32(one, 5, one, one, fh, ch, 2, 12, 2, 1, one, None) == -1 and b'mode' in lib.bdv_last_error()
    counts[1] = 0
    assert lib.bdv_temporal_nanreduce_f32(one, 5, one, one, fh, ch, 2, 12, 0, 1, one, None) == -1 and b'video 1' in lib.bdv_last_error()


def test_python_argument_errors(tmp_path):
    jobs = [(str(tmp_path / 'v'), str(tmp_path / 'v.jpg'))]
    with pytest.raises(ValueError, match='method'):
        BG.extract_backgrounds(jobs, method='median')
    with pytest.raises(ValueError, match='avg_method'):
        BG.extract_backgrounds(jobs, method='sim_cam', avg_method='mode')
    with pytest.raises(ValueError, match='tmf'):
        BG.extract_backgrounds(jobs, method='tmf', avg_method='mean')
    with pytest.raises(ValueError, match='tmf'):
        BG.extract_backgrounds(jobs, interval=2)
    with pytest.raises(ValueError, match='tmf'):
        BG.extract_background(*jobs[0], max_frames=100)
    with pytest.raises(ValueError, match='avg_method'):
        BG.temporal_nanreduce(np.zeros((2, 3), np.float32), [2], avg_method='max')
    with pytest.raises(ValueError, match='float32'):
        BG.temporal_nanreduce(np.zeros((2, 3), np.float64), [2])
    with pytest.raises(ValueError, match='partition'):
        BG.temporal_nanreduce(np.zeros((4, 3), np.float32), [3, 2])
    with pytest.raises(ValueError, match='partition'):
        BG.temporal_nanreduce(np.zeros((4, 3), np.float32), [4, 0])
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match='boxes'):
        BG.resized_crop(frames, [(0, 0, 8, 8)])
    with pytest.raises(ValueError, match='leaves'):
        BG.resized_crop(frames, [(0, 0, 8, 8), (1, 0, 8, 8)])
    with pytest.raises(ValueError, match='leaves'):
        BG.resized_crop(frames, [(0, 0, 8, 8), (0, 0, 0, 8)])
    with pytest.raises(ValueError, match='uint8'):
        BG.resized_crop(frames.astype(np.float32), [(0, 0, 8, 8)] * 2)


def test_cli_parser_defaults_and_from_video(tmp_path, capsys):
    from tools import extract_background as CLI
    a = CLI.build_parser().parse_args(['--video_dir', 'v', '--output_dir', 'o'])
    assert (a.glob_pattern, a.num_workers, a.from_video, a.image_suffix, a.interval, a.max_frames, a.size, a.method, a.avg_method) == \
        ('*', 4, False, '.jpg', 1, 500, 256, 'tmf', 'median')                  # the reference's defaults
    assert (a.sim_cam_size, a.antialias, a.seed) == (100, False, None)
    a = CLI.build_parser().parse_args(['--video_dir', 'v', '--output_dir', 'o', '--method', 'sim_cam', '--avg_method', 'mean', '--seed', '3',
                                       '--antialias', '--sim_cam_size', '64', '--interval', '2', '--max_frames', '50', '--size', '1'])
    assert (a.method, a.avg_method, a.seed, a.antialias, a.sim_cam_size, a.interval, a.max_frames) == ('sim_cam', 'mean', 3, True, 64, 2, 50)
    with pytest.raises(SystemExit):
        CLI.build_parser().parse_args(['--video_dir', 'v', '--output_dir', 'o', '--method', 'other'])
    out = tmp_path / 'bg'
    with pytest.raises(SystemExit) as e:
        CLI.main(['--video_dir', str(tmp_path), '--output_dir', str(out), '--from_video'])
    assert e.value.code != 0 and 'video decoder' in capsys.readouterr().err
    assert not out.exists()
    # the skip rule and the two printed counts, on a run with nothing left to do (no GPU is touched)
    vids = tmp_path / 'frames'
    for n in ('v_a', 'v_b.avi'):
        (vids / n).mkdir(parents=True)
    out.mkdir()
    for n in ('v_a.jpg', 'v_b.jpg'):
        (out / n).write_bytes(b'existing')
    found, todo = CLI.pending_videos(vids, '*', out, '.jpg')
    assert [p.name for p in found] == ['v_a', 'v_b.avi'] and todo == []
    found, todo = CLI.pending_videos(vids, 'v_a*', out, '.png')
    assert found == [] and [p.name for p in todo] == ['v_a']
    assert CLI.main(['--video_dir', str(vids), '--output_dir', str(out), '--method', 'sim_cam']) == 0
    assert capsys.readouterr().out.splitlines() == ['Found 2 backgrounds', 'Extracting background from 0 videos']
