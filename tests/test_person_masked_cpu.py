"""``method='person_masked'`` without a GPU: the box table, the frame selection, the argument checks of every layer (Python, C entry
point, config, command line), the report file and its "do not retry a rejected video" rule, and the ABI."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest

import bdvcil_amd as bd
from bdvcil_amd import background as BG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cil_configs.json')
BGMIX = 'ucf101/bgmix_plus_randAug/bgmix_seed_1000_inc_10_stages_bgmix_plus_randAug.py'
ACM = 'ucf101/seed_1000_inc_10_stages_ActorCutMix_plus_randAug.py'
NAME = 'bdv_temporal_masked_median_u8'


def _rows(*rows):
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


# ---- person_box_table ---------------------------------------------------------------------------------------------------------------
def test_box_table_threshold_indexing_and_csr():
    dets = [_rows([0, 0, 10, 10, 0.99]),                                   # entry 0: no 1-based frame number reads it
            _rows([10, 20, 30, 40, 0.4], [50, 10, 60, 30, 0.41]),          # a score of exactly det_thres is dropped (strict >)
            _rows(),                                                       # an entry without rows
            _rows([10, 20, 30, 40, 0.9], [12, 22, 28, 38, 0.5], [1, 1, 2, 2, 0.1])]
    box_first, boxes, have = BG.person_box_table(dets, [1, 2, 3, 4, 9], 100, 80, det_thres=0.4, dilate=0.0)
    assert box_first.dtype == np.int32 and boxes.dtype == np.int32 and have.dtype == bool
    assert box_first.tolist() == [0, 1, 1, 3, 3, 3]                        # frame 1: one row; 2: none; 3: two; 4 and 9: past the list's end
    assert boxes.tolist() == [[50, 10, 60, 30], [10, 20, 30, 40], [12, 22, 28, 38]]
    assert have.tolist() == [True, True, True, False, False]
    # frame number i reads entry i: number 0 reads the entry the datasets never reach
    assert BG.person_box_table(dets, [0], 100, 80, dilate=0.0)[1].tolist() == [[0, 0, 10, 10]]
    empty = BG.person_box_table(dets, [2], 100, 80)
    assert empty[0].tolist() == [0, 0] and empty[1].shape == (0, 4) and empty[2].tolist() == [True]
    assert BG.person_box_table(dets, [], 100, 80)[0].tolist() == [0]


def test_box_table_dilation_rounding_and_clipping():
    W, H = 100, 80

    def one(box, dilate=0.1):
        return BG.person_box_table([_rows([*box, 0.9])], [0], W, H, dilate=dilate)[1].tolist()

    # 20 x 20 grown by 2 on every side; whole numbers stay as they are
    assert one([30, 30, 50, 50]) == [[28, 28, 52, 52]]
    # fractional: (10.5, 20.25, 30.75, 40.5) is 20.25 x 20.25, grows by 2.025 -> (8.475, 18.225, 32.775, 42.525) -> floor / ceil
    assert one([10.5, 20.25, 30.75, 40.5]) == [[8, 18, 33, 43]]
    # without dilation a partly covered pixel still counts: floor of the near edges, ceil of the far ones
    assert one([10.5, 20.25, 30.75, 40.5], 0.0) == [[10, 20, 31, 41]]
    # clipped at the left and top, at the right and bottom
    assert one([1, 1, 21, 11]) == [[0, 0, 23, 12]]
    assert one([85, 65, 99, 79]) == [[83, 63, 100, 80]]
    assert one([-50, -50, 500, 500], 0.0) == [[0, 0, W, H]]
    # boxes left empty are dropped: outside the frame, and of no width
    assert one([120, 10, 140, 30]) == [] and one([10, -30, 20, -10]) == [] and one([40, 10, 40, 30]) == []
    # the box's own width and height scale the growth: 40 x 10 grows by 4 and by 1
    assert one([30, 30, 70, 40]) == [[26, 29, 74, 41]]


# ---- frame selection ----------------------------------------------------------------------------------------------------------------
def test_template_frame_files(tmp_path):
    d = tmp_path / 'v_x'
    d.mkdir()
    for n in ('img_00002.jpg', 'img_00001.jpg', 'img_00010.jpg', 'flow_x_00001.jpg', 'flow_y_00001.jpg', 'notes.txt', 'img_3.jpg',
              'img_00004.jpg.bak', 'ximg_00005.jpg'):
        (d / n).write_bytes(b'x')
    (d / 'img_00007.jpg').mkdir()                                            # not a file
    got = BG.template_frame_files(d)
    assert [(i, p.name) for i, p in got] == [(1, 'img_00001.jpg'), (2, 'img_00002.jpg'), (10, 'img_00010.jpg')]
    assert [(i, p.name) for i, p in BG.template_frame_files(d, 'flow_x_{:05d}.jpg')] == [(1, 'flow_x_00001.jpg')]
    assert [(i, p.name) for i, p in BG.template_frame_files(d, 'img_{}.jpg')] == [(3, 'img_3.jpg')]
    with pytest.raises(ValueError, match='filename_tmpl'):
        BG.template_frame_files(d, 'img.jpg')
    with pytest.raises(FileNotFoundError):
        BG.template_frame_files(tmp_path / 'nowhere')


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_check_method_matrix():
    ok = ('median', 1, BG.SIM_CAM_MAX_FRAMES)
    assert BG.METHODS == ('tmf', 'sim_cam', 'person_masked')
    BG._check_method('tmf', *ok)
    BG._check_method('sim_cam', 'mean', 2, 50)
    BG._check_method('person_masked', *ok, det_file='d.npy')
    BG._check_method('person_masked', *ok, det_file='d.npy', det_thres=0.5, dilate=0.0, min_visible=3, max_hole_fraction=0.25,
                     filename_tmpl='image_{:05d}.jpg', report=[])
    new = dict(det_file='d.npy', det_thres=0.5, dilate=0.2, min_visible=2, max_hole_fraction=0.1, filename_tmpl='f_{}.jpg', report=[])
    for method, args in (('tmf', ok), ('sim_cam', ('mean', 2, 50))):
        for key, value in new.items():                                       # each new keyword on its own is refused by the other methods
            with pytest.raises(ValueError, match=key):
                BG._check_method(method, *args, **{key: value})
    with pytest.raises(ValueError, match='det_file'):
        BG._check_method('person_masked', *ok)
    for bad in (('mean', 1, BG.SIM_CAM_MAX_FRAMES), ('median', 2, BG.SIM_CAM_MAX_FRAMES), ('median', 1, 100)):
        with pytest.raises(ValueError, match='sim_cam'):
            BG._check_method('person_masked', *bad, det_file='d.npy')
    for key, value in (('min_visible', 0), ('dilate', -0.1), ('max_hole_fraction', 1.5), ('report', {})):
        with pytest.raises(ValueError, match=key):
            BG._check_method('person_masked', *ok, det_file='d.npy', **{key: value})
    with pytest.raises(ValueError, match='method'):
        BG._check_method('mask_rcnn', *ok)
    # through the public entry points, before anything is read or decoded
    with pytest.raises(ValueError, match='det_file'):
        BG.extract_backgrounds([('nowhere', 'x.jpg')], method='person_masked')
    with pytest.raises(ValueError, match='det_file'):
        BG.extract_backgrounds([('nowhere', 'x.jpg')], det_file='d.npy')
    with pytest.raises(ValueError, match='min_visible'):
        BG.extract_background('nowhere', 'x.jpg', method='sim_cam', min_visible=2)


def test_masked_median_argument_errors_launch_nothing(monkeypatch):
    from bdvcil_amd import kernels as K
    monkeypatch.setattr(K, 'temporal_masked_median_u8', lambda *a, **k: pytest.fail('the kernel wrapper was reached'))
    frames = np.zeros((3, 4, 6, 3), np.uint8)
    good_first, good_boxes = [0, 1, 1, 2], [[0, 0, 6, 4], [1, 1, 1, 1]]
    with pytest.raises(ValueError, match='box_first'):
        BG.temporal_masked_median(frames, [3], [0, 2, 1, 2], good_boxes)                       # decreases
    with pytest.raises(ValueError, match='box_first'):
        BG.temporal_masked_median(frames, [3], [0, 1, 2], good_boxes)                          # one entry per frame, plus one
    with pytest.raises(ValueError, match='box_first'):
        BG.temporal_masked_median(frames, [3], [0, 1, 1, 3], good_boxes)                       # past the rows
    for bad in ([0, 0, 7, 4], [0, 0, 6, 5], [-1, 0, 6, 4], [0, -1, 6, 4], [3, 0, 2, 4], [0, 3, 6, 2]):
        with pytest.raises(ValueError, match='box'):
            BG.temporal_masked_median(frames, [3], good_first, [bad, [1, 1, 1, 1]])
    with pytest.raises(ValueError, match='min_visible'):
        BG.temporal_masked_median(frames, [3], good_first, good_boxes, min_visible=0)
    with pytest.raises(ValueError, match='65535'):
        BG.temporal_masked_median(np.zeros((65536, 1, 1, 3), np.uint8), [65536], np.zeros(65537, np.int32), np.zeros((0, 4), np.int32))
    with pytest.raises(ValueError, match='partition'):
        BG.temporal_masked_median(frames, [2, 2], good_first, good_boxes)
    with pytest.raises(ValueError, match='uint8'):
        BG.temporal_masked_median(frames.astype(np.float32), [3], good_first, good_boxes)


def test_entry_point_rejects_bad_tables_before_any_launch():
    lib = bd._lib.lib()
    one = ctypes.c_void_p(16)           # never dereferenced: the calls fail on their host arguments
    first, counts = (ctypes.c_int64 * 2)(0, 2), (ctypes.c_int32 * 2)(2, 1)
    box_first, boxes = (ctypes.c_int32 * 4)(0, 1, 1, 2), (ctypes.c_int32 * 8)(0, 0, 6, 4, 1, 1, 1, 1)
    fh, ch, bfh, bxh = (ctypes.cast(a, ctypes.c_void_p) for a in (first, counts, box_first, boxes))

    def call(total=3, V=2, H=4, W=6, nb=2, min_visible=1, bx=one):
        code = lib.bdv_temporal_masked_median_u8(one, total, one, one, fh, ch, V, H, W, one, bx, bfh, bxh, nb, min_visible, one, one, None)
        return code, lib.bdv_last_error()

    code, err = call(min_visible=0)
    assert code == -1 and b'min_visible' in err
    code, err = call(W=5)
    assert code == -1 and b'box 0' in err and b'not inside' in err
    boxes[4], boxes[6] = 3, 2                                                 # x0 > x1
    code, err = call()
    assert code == -1 and b'box 1' in err
    boxes[4], boxes[6] = 1, 1
    box_first[1], box_first[2] = 2, 1
    code, err = call()
    assert code == -1 and b'decreases at frame 1' in err
    box_first[1], box_first[2] = 1, 1
    code, err = call(nb=1)
    assert code == -1 and b'box_first' in err
    counts[0] = 65536
    code, err = call(total=65537)
    assert code == -1 and b'video 0' in err
    counts[0] = 2
    code, err = call(bx=ctypes.c_void_p(8))
    assert code == -1 and b'aligned' in err


def test_abi_symbol_and_version():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read(), flags=re.S)
    m = re.search(r'^int\s+' + NAME + r'\s*\((.*?)\);', hdr, re.S | re.M)
    assert m, f'{NAME} is not declared in include/bdvcil_hip.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert hasattr(ctypes.CDLL(bd._lib.LIB_PATH), NAME), f'{NAME} is not exported by the built library'
    res, args = bd._lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == len(params)
    for p, a in zip(params, args):                                            # pointers against pointers, scalars against scalars
        assert ('*' in p) == (a is bd._lib.P), (p, a)
    assert bd._lib.ABI_VERSION == 33 and bd._lib.lib().bdv_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read()
    assert 'cil_tools/type_b_and_c_bg.py:47-54' in raw and 'libs/loader/comix_loader.py:148-164' in raw
    for name in ('person_box_table', 'temporal_masked_median'):
        assert getattr(bd, name) is getattr(BG, name)


# ---- the report file ----------------------------------------------------------------------------------------------------------------
def test_report_round_trip_and_no_retry_of_rejected_videos(tmp_path, monkeypatch):
    bg = tmp_path / 'bg'
    infos = [dict(frame_dir=str(tmp_path / 'frames' / n), total_frames=5, label=0) for n in ('v_a', 'v_b', 'v_c')]
    calls = []

    def stub(jobs, decoder=None, quality=95, max_batch_bytes=0, report=None, **kw):
        """Writes v_a and v_c, rejects v_b."""
        calls.append(([os.path.basename(d) for d, _ in jobs], kw))
        for d, dest in jobs:
            written = not d.endswith('v_b')
            if written:
                with open(dest, 'wb') as f:
                    f.write(b'jpeg')
            report.append(dict(frame_dir=d, dest=dest, frames=5, frames_without_entry=1, boxes=4, hole_fraction=0.0 if written else 0.25,
                               written=written))

    monkeypatch.setattr(BG, 'extract_backgrounds', stub)
    ext = dict(method='person_masked', det_file='det.npy', max_hole_fraction=0.1)
    real = os.path.realpath(bg)
    out = BG.resolve_bg_files(infos, str(bg), bg_extraction=ext)
    assert out == [os.path.join(real, 'v_a.jpg'), os.path.join(real, 'v_c.jpg')]
    assert calls == [(['v_a', 'v_b', 'v_c'], ext)]
    rep = json.loads((bg / BG.REPORT_NAME).read_text())
    assert rep == BG.load_person_masked_report(bg)
    assert rep['params'] == dict(det_file='det.npy', det_thres=0.4, dilate=0.1, min_visible=1, max_hole_fraction=0.1,
                                 filename_tmpl='img_{:05}.jpg')
    assert sorted(rep['videos']) == ['v_a.jpg', 'v_b.jpg', 'v_c.jpg']
    assert rep['videos']['v_b.jpg'] == dict(frame_dir=infos[1]['frame_dir'], dest=os.path.join(real, 'v_b.jpg'), frames=5,
                                            frames_without_entry=1, boxes=4, hole_fraction=0.25, written=False)
    assert sorted(p.name for p in bg.iterdir()) == [BG.REPORT_NAME, 'v_a.jpg', 'v_c.jpg']          # no temporary file left
    # again: nothing is missing but the rejected video, which is on record -> no extraction at all
    assert BG.resolve_bg_files(infos, str(bg), bg_extraction=ext) == out and len(calls) == 1
    # a written file that disappeared is made again, the rejected one still is not; the record keeps all three
    os.unlink(bg / 'v_c.jpg')
    assert BG.resolve_bg_files(infos, str(bg), bg_extraction=ext) == out and calls[1][0] == ['v_c']
    assert sorted(BG.load_person_masked_report(bg)['videos']) == ['v_a.jpg', 'v_b.jpg', 'v_c.jpg']
    # other parameters: the record does not apply, the rejected video is tried again, and the old rows go
    ext2 = dict(ext, max_hole_fraction=0.2)
    BG.resolve_bg_files(infos, str(bg), bg_extraction=ext2)
    assert calls[2] == (['v_b'], ext2)
    rep = BG.load_person_masked_report(bg)
    assert rep['params']['max_hole_fraction'] == 0.2 and sorted(rep['videos']) == ['v_b.jpg']
    # the report is not a background
    assert BG.resolve_bg_files(infos, str(bg), map_bg_to_video=False) == [os.path.join(real, 'v_a.jpg'), os.path.join(real, 'v_c.jpg')]
    # an unreadable report counts as none
    (bg / BG.REPORT_NAME).write_text('{ truncated')
    assert BG.load_person_masked_report(bg) is None
    BG.resolve_bg_files(infos, str(bg), bg_extraction=ext2)
    assert calls[3][0] == ['v_b']
    # without the key: today's call, no report keyword
    os.unlink(bg / BG.REPORT_NAME)
    os.unlink(bg / 'v_a.jpg')
    seen = []
    monkeypatch.setattr(BG, 'extract_backgrounds', lambda *a, **k: seen.append((a[1:], k)))
    BG.resolve_bg_files(infos, str(bg))
    assert seen == [((None, BG.DEFAULT_QUALITY, BG.MAX_BATCH_BYTES), {})] and not (bg / BG.REPORT_NAME).exists()


# ---- config -------------------------------------------------------------------------------------------------------------------------
def test_config_key(monkeypatch):
    from bdvcil_amd.config_run import bg_extraction_spec, clip_loader_spec
    with open(GOLDEN) as f:
        configs = json.load(f)
    plain = clip_loader_spec(configs[BGMIX])
    assert 'bg_extraction' not in plain['dataset']
    assert sorted(plain['dataset']) == ['back_ground_from_bg_dir', 'bg_dir', 'bg_image_extension', 'extract_bg_if_not_found', 'map_bg_to_video',
                                        'merge_bg_files', 'type']
    assert bg_extraction_spec(configs[BGMIX]['data']['train']) is None

    def with_key(ext, name=BGMIX):
        cfg = copy.deepcopy(configs[name])
        cfg['data']['train']['bg_extraction'] = ext
        return cfg

    ext = dict(method='person_masked', det_file='data/det.npy', det_thres=0.5, dilate=0.05, min_visible=2, max_hole_fraction=0.02)
    spec = clip_loader_spec(with_key(ext))
    assert spec['dataset']['bg_extraction'] == dict(ext, filename_tmpl=spec['kwargs']['filename_tmpl'])
    assert {k: v for k, v in spec['dataset'].items() if k != 'bg_extraction'} == plain['dataset']          # nothing else moves
    assert spec['kwargs'] == plain['kwargs'] and spec['loader'] == plain['loader']
    assert clip_loader_spec(with_key(dict(method='person_masked', det_file='d.npy', filename_tmpl='image_{:05d}.jpg'))
                            )['dataset']['bg_extraction']['filename_tmpl'] == 'image_{:05d}.jpg'
    assert clip_loader_spec(with_key(dict(method='tmf')))['dataset']['bg_extraction'] == dict(method='tmf')
    with pytest.raises(ValueError, match=r'bg_extraction method.*mask_rcnn'):
        clip_loader_spec(with_key(dict(method='mask_rcnn', det_file='d.npy')))
    with pytest.raises(ValueError, match=r'bg_extraction threshold.*unknown key'):
        clip_loader_spec(with_key(dict(method='person_masked', det_file='d.npy', threshold=0.5)))
    with pytest.raises(ValueError, match=r'bg_extraction det_file.*missing'):
        clip_loader_spec(with_key(dict(method='person_masked', det_thres=0.5)))
    with pytest.raises(ValueError, match=r'bg_extraction det_file'):
        clip_loader_spec(with_key(dict(method='sim_cam', det_file='d.npy')))
    with pytest.raises(ValueError, match='bg_extraction'):
        clip_loader_spec(with_key('person_masked'))
    with pytest.raises(ValueError, match='bg_extraction'):
        clip_loader_spec(with_key(ext, ACM))                                  # no bg_dir to fill


def test_task_loop_hands_the_key_to_both_resolve_calls(monkeypatch):
    """``CILTaskLoop._train_records`` on stand-ins: rank 0 extracts with the key, the other ranks resolve with it after the barrier;
    without the key the calls are today's."""
    import bdvcil_amd.task_loop as TL
    seen = []
    monkeypatch.setattr(BG, 'resolve_bg_files', lambda infos, bg_dir, **kw: seen.append(kw) or [])
    monkeypatch.setattr(TL, 'RawframeRecords', lambda *a, **k: type('R', (), dict(video_infos=[], bg_files=[], merge_bg_files=True))())
    ext = dict(method='person_masked', det_file='d.npy', max_hole_fraction=0.0)
    for rank in (0, 1):
        for train in (dict(bg_dir='bg'), dict(bg_dir='bg', bg_extraction=ext, filename_tmpl='image_{:05d}.jpg')):
            loop = object.__new__(TL.CILTaskLoop)
            loop.config, loop.rank, loop.world = TL.AttrDict(dict(data=dict(train=train), data_root='r')), rank, 1
            loop._train_records('ann.txt')
    base = dict(map_bg_to_video=True, bg_image_extension='.jpg')
    full = dict(ext, filename_tmpl='image_{:05d}.jpg')
    assert seen == [dict(base, extract_bg_if_not_found=True), dict(base, extract_bg_if_not_found=True, bg_extraction=full),
                    dict(base, extract_bg_if_not_found=False), dict(base, extract_bg_if_not_found=False, bg_extraction=full)]


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path, capsys):
    from tools import extract_background as CLI
    base = ['--video_dir', 'v', '--output_dir', 'o']
    _, a = CLI.parse_args(base)
    assert (a.method, a.det_file, a.det_thres, a.dilate, a.min_visible, a.max_hole_fraction, a.filename_tmpl) == \
        ('tmf', None, 0.4, 0.1, 1, None, 'img_{:05}.jpg')
    _, a = CLI.parse_args(base + ['--method', 'person_masked', '--det_file', 'd.npy', '--det_thres', '0.5', '--dilate', '0', '--min_visible', '3',
                                  '--max_hole_fraction', '0.05', '--filename_tmpl', 'image_{:05d}.jpg'])
    assert (a.method, a.det_file, a.det_thres, a.dilate, a.min_visible, a.max_hole_fraction, a.filename_tmpl) == \
        ('person_masked', 'd.npy', 0.5, 0.0, 3, 0.05, 'image_{:05d}.jpg')
    for argv, word in ((base + ['--det_file', 'd.npy'], '--det_file'), (base + ['--method', 'sim_cam', '--det_file', 'd.npy'], '--det_file'),
                       (base + ['--min_visible', '2'], '--min_visible'), (base + ['--method', 'person_masked'], '--det_file')):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    out = tmp_path / 'bg'
    with pytest.raises(SystemExit):
        CLI.main(['--video_dir', str(tmp_path), '--output_dir', str(out), '--det_file', 'd.npy'])
    assert not out.exists()                                                   # refused before anything is made
