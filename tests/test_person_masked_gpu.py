"""The person-masked temporal median on the GPU against its numpy oracle (tests/person_masked_oracle.py), and
``method='person_masked'`` end to end: frame directories and a detection file made here, the written files against the oracle applied
to the decoded frames.  Every kernel result is compared with ``==``."""
import json
import os
import pathlib

import numpy as np
import pytest
import torch

import person_masked_oracle as PO
from bdvcil_amd import background as BG

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 7, 34)
# (family, frames, a box over the whole first frame): every count in both the noise and the narrow family, the straddling stacks at
# the even counts
VIDEOS = [(fam, F, (i + j) % 2 == 0) for i, fam in enumerate(('noise', 'narrow')) for j, F in enumerate(COUNTS)] + \
         [(fam, F, F == 34) for fam in ('mid15_16', 'mid127_128') for F in (2, 34)]
_cache = {}


def _batch(hw):
    """One ragged batch per geometry and its oracle results per ``min_visible``, computed once and shared (read only)."""
    if hw not in _cache:
        H, W = hw
        rng = np.random.default_rng(H * 100 + W)
        stacks = [PO.value_stack(fam, F, H, W, rng) for fam, F, _ in VIDEOS]
        boxes = [PO.edge_boxes(F, H, W, whole) for _, F, whole in VIDEOS]
        ref = {mv: [PO.masked_median(s, b, mv) for s, b in zip(stacks, boxes)] for mv in (1, 3)}
        for a in stacks:
            a.setflags(write=False)
        _cache[hw] = stacks, boxes, ref
    return _cache[hw]


@pytest.mark.parametrize('min_visible', [1, 3])
@pytest.mark.parametrize('hw', [(5, 7), (6, 8)])          # 105 bytes per frame: the unaligned path with a partial last group; 144: aligned
def test_masked_median_matches_oracle(dev, hw, min_visible):
    stacks, boxes, ref = _batch(hw)
    box_first, rows = PO.box_table(boxes)
    out, visible = BG.temporal_masked_median(torch.from_numpy(np.concatenate(stacks)).to(dev), [len(s) for s in stacks], box_first, rows,
                                             min_visible)
    assert out.dtype == torch.uint8 and visible.dtype == torch.uint16
    out, visible = out.cpu().numpy(), visible.cpu().numpy()
    want_vis = np.stack([r[1] for r in ref[min_visible]])
    # the batch holds what it is meant to hold
    assert (want_vis == 0).any() and (want_vis == min_visible).any() and (want_vis == min_visible - 1).any()
    assert ((want_vis >= min_visible) & (want_vis % 2 == 0)).any() and ((want_vis >= min_visible) & (want_vis % 2 == 1)).any()
    for v, (want, vis) in enumerate(ref[min_visible]):
        np.testing.assert_array_equal(visible[v], vis, err_msg=f'visible, video {v} {VIDEOS[v]}')
        np.testing.assert_array_equal(out[v], want, err_msg=f'out, video {v} {VIDEOS[v]}')


@pytest.mark.parametrize('hw', [(5, 7), (6, 8)])
def test_grouped_oracle_is_the_pixel_oracle(hw):
    stacks, boxes, ref = _batch(hw)
    for mv in (1, 3):
        for s, b, (want, vis) in zip(stacks, boxes, ref[mv]):
            got, gvis = PO.masked_median_grouped(s, b, mv)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(gvis, vis)


@pytest.mark.parametrize('hw', [(5, 7), (6, 8), (31, 23)])
def test_empty_table_is_the_plain_median(dev, hw):
    stacks = _batch(hw)[0] if hw in ((5, 7), (6, 8)) else \
        [np.random.default_rng(3).integers(0, 256, (F, *hw, 3), dtype=np.uint8) for F in COUNTS]
    counts = [len(s) for s in stacks]
    frames = torch.from_numpy(np.concatenate(stacks)).to(dev)
    out, visible = BG.temporal_masked_median(frames, counts, np.zeros(sum(counts) + 1, np.int32), np.zeros((0, 4), np.int32), 1)
    assert torch.equal(out, BG.temporal_median(frames, counts))
    want = torch.tensor(counts, dtype=torch.int32).view(-1, 1, 1).expand(-1, *hw)
    assert torch.equal(visible.cpu().to(torch.int32), want)


def test_masked_median_many_workgroups(dev):
    """240 x 320: 225 workgroups per video.  A person who never leaves (holes), one who walks, and a frame-wide box."""
    H, W, F = 240, 320, 40
    rng = np.random.default_rng(11)
    stacks = [rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8), rng.integers(100, 104, (F, H, W, 3), dtype=np.uint8),
              PO.value_stack('mid127_128', F, H, W, rng)]
    boxes = []
    for v in range(3):
        per_frame = []
        for f in range(F):
            rows = [[100 + 4 * f, 50, 150 + 4 * f, 200]]                    # walks 4 pixels a frame
            if v != 1:
                rows.append([201, 101, 231, 239])                           # never moves: holes, odd edges
            if v == 2 and f % 2 == 0:
                rows.append([0, 0, W, H])
            per_frame.append(np.asarray(rows, dtype=np.int32))
        boxes.append(per_frame)
    box_first, rows = PO.box_table(boxes)
    out, visible = BG.temporal_masked_median(torch.from_numpy(np.concatenate(stacks)).to(dev), [F] * 3, box_first, rows, 2)
    out, visible = out.cpu().numpy(), visible.cpu().numpy()
    for v in range(3):
        want, vis = PO.masked_median_grouped(stacks[v], boxes[v], 2)
        np.testing.assert_array_equal(visible[v], vis, err_msg=f'visible, video {v}')
        np.testing.assert_array_equal(out[v], want, err_msg=f'out, video {v}')
    assert (visible[0] == 0).any() and (visible[1] == F).any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
H, W, F = 48, 64, 10
RECT_A, RECT_B, RECT_S = (8, 10, 24, 34), (40, 10, 56, 34), (20, 12, 36, 36)      # x0, y0, x1, y1; 16 x 24 each
DET = dict(det_thres=0.4, dilate=0.1)


def _dilated(r):
    w, h = r[2] - r[0], r[3] - r[1]
    return (int(np.floor(r[0] - 0.1 * w)), int(np.floor(r[1] - 0.1 * h)), int(np.ceil(r[2] + 0.1 * w)), int(np.ceil(r[3] + 0.1 * h)))


def _texture(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 90 * np.sin(xx / 5.0), 128 + 90 * np.cos(yy / 4.0), (5 * xx + 3 * yy) % 256], -1) + rng.normal(0, 10, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def scene(dev, tmp_path_factory):
    """Two frame directories and their detection file: ``v_moving`` -- the rectangle at RECT_A in 6 of 10 frames, at RECT_B in the
    others; ``v_static`` -- at RECT_S in every frame.  Each directory also holds a flow frame and a stray file."""
    tmp = tmp_path_factory.mktemp('person_masked')
    root = tmp / 'rawframes'
    dets, clean = {}, {}
    for name, seed in (('v_moving', 1), ('v_static', 2)):
        d = root / name
        d.mkdir(parents=True)
        clean[name] = _texture(seed)
        frames, per_frame = [], [np.zeros((0, 5), dtype=np.float32)]             # entry 0 is never read (1-based numbers)
        for i in range(1, F + 1):
            r = RECT_S if name == 'v_static' else (RECT_A if i % 5 < 3 else RECT_B)      # i % 5 in (0, 1, 2): 6 of 10 frames
            frame = clean[name].copy()
            frame[r[1]:r[3], r[0]:r[2]] = (200, 30, 30)
            frames.append(frame)
            per_frame.append(np.asarray([[*r, 0.9], [0, 0, W, H, 0.3]], dtype=np.float32))      # the decoy is below the threshold
        dets[name] = per_frame
        for i, data in enumerate(BG.encode_jpeg(np.stack(frames), 90), start=1):
            (d / f'img_{i:05}.jpg').write_bytes(data)
        (d / 'flow_x_00001.jpg').write_bytes((d / 'img_00001.jpg').read_bytes())
        (d / 'notes.txt').write_text('not a frame')
    det_file = tmp / 'detections.npy'
    np.save(det_file, dets, allow_pickle=True)
    return dict(tmp=tmp, root=root, det_file=str(det_file), dets=dets, clean=clean)


class CountingDecoder:
    def __init__(self):
        from bdvcil_amd.decode import JpegDecoder
        self.inner, self.calls = JpegDecoder('cuda', threads=4), 0
        self.device, self.threads = self.inner.device, self.inner.threads

    def decode(self, streams):
        self.calls += 1
        return self.inner.decode(streams)


def _oracle_background(scene, name, min_visible=1):
    from bdvcil_amd.decode import JpegDecoder
    files = [scene['root'] / name / f'img_{i:05}.jpg' for i in range(1, F + 1)]
    decoded = JpegDecoder('cuda', threads=4).decode([p.read_bytes() for p in files]).cpu().numpy()
    box_first, rows, have = BG.person_box_table(scene['dets'][name], range(1, F + 1), W, H, **DET)
    assert have.all()
    per_frame = [rows[box_first[k]:box_first[k + 1]] for k in range(F)]
    return PO.masked_median(decoded, per_frame, min_visible)


def _infos(scene):
    return [dict(frame_dir=str(scene['root'] / n), total_frames=F, label=k) for k, n in enumerate(('v_moving', 'v_static'))]


def test_person_masked_end_to_end(dev, scene):
    tmp = scene['tmp']
    bg = pathlib.Path(os.path.realpath(tmp)) / 'bg'
    ext = dict(method='person_masked', det_file=scene['det_file'], max_hole_fraction=0.0, **DET)
    decoder = CountingDecoder()
    out = BG.resolve_bg_files(_infos(scene), str(bg), decoder=decoder, bg_extraction=ext)
    assert out == [str(bg / 'v_moving.jpg')] and decoder.calls > 0                 # v_static is rejected: its person never moves
    want, vis = _oracle_background(scene, 'v_moving')
    assert (bg / 'v_moving.jpg').read_bytes() == BG.encode_jpeg(want[None])[0]
    assert sorted(p.name for p in bg.iterdir()) == [BG.REPORT_NAME, 'v_moving.jpg']

    rows = json.loads((bg / BG.REPORT_NAME).read_text())['videos']
    a, s = _dilated(RECT_A), _dilated(RECT_S)
    assert rows['v_moving.jpg']['written'] and rows['v_moving.jpg']['hole_fraction'] == 0.0 and (vis > 0).all()
    assert rows['v_moving.jpg']['frames'] == F and rows['v_moving.jpg']['frames_without_entry'] == 0 and rows['v_moving.jpg']['boxes'] == F
    assert not rows['v_static.jpg']['written']
    assert rows['v_static.jpg']['hole_fraction'] == (s[2] - s[0]) * (s[3] - s[1]) / (H * W)

    # the person is gone where the plain median keeps it: inside the 60 % region the masked background is closer to the clean one
    only_frames = tmp / 'tmf_frames' / 'v_moving'                             # 'tmf' reads every file of a directory
    only_frames.mkdir(parents=True)
    for p in (scene['root'] / 'v_moving').glob('img_*.jpg'):
        (only_frames / p.name).write_bytes(p.read_bytes())
    tmf = BG.extract_background(only_frames, tmp / 'tmf' / 'v_moving.jpg').astype(np.int32)
    clean = scene['clean']['v_moving'].astype(np.int32)
    region = np.s_[a[1]:a[3], a[0]:a[2]]
    assert np.abs(want.astype(np.int32) - clean)[region].mean() < np.abs(tmf - clean)[region].mean()

    # a second call decodes nothing: v_moving exists, v_static is on record as rejected under these parameters
    calls = decoder.calls
    assert BG.resolve_bg_files(_infos(scene), str(bg), decoder=decoder, bg_extraction=ext) == out and decoder.calls == calls
    # other parameters: the record no longer applies, and without the limit the static video is written, holes filled by the plain median
    ext2 = dict(ext, max_hole_fraction=None)
    out2 = BG.resolve_bg_files(_infos(scene), str(bg), decoder=decoder, bg_extraction=ext2)
    assert out2 == [str(bg / 'v_moving.jpg'), str(bg / 'v_static.jpg')] and decoder.calls > calls
    assert (bg / 'v_static.jpg').read_bytes() == BG.encode_jpeg(_oracle_background(scene, 'v_static')[0][None])[0]


def test_extract_backgrounds_report_and_errors(dev, scene):
    tmp = scene['tmp'] / 'direct'
    report = []
    jobs = [(str(scene['root'] / n), str(tmp / f'{n}.jpg')) for n in ('v_static', 'v_moving')]
    arrays = BG.extract_backgrounds(jobs, return_arrays=True, method='person_masked', det_file=scene['det_file'], min_visible=5,
                                    report=report, **DET)
    assert [r['frame_dir'] for r in report] == [j[0] for j in jobs] and all(r['written'] for r in report)
    a, b = _dilated(RECT_A), _dilated(RECT_B)
    # with min_visible = 5 the 60 % region (seen in 4 frames) is a hole too, the 40 % region (seen in 6) is not
    assert report[1]['hole_fraction'] == (a[2] - a[0]) * (a[3] - a[1]) / (H * W) and (b[2] - b[0]) > 0
    for (n, arr) in zip(('v_static', 'v_moving'), arrays):
        np.testing.assert_array_equal(arr, _oracle_background(scene, n, 5)[0])
    # a video the detection file does not list: named, and nothing of the call is written
    other = scene['root'] / 'v_unlisted'
    other.mkdir()
    (other / 'img_00001.jpg').write_bytes((scene['root'] / 'v_moving' / 'img_00001.jpg').read_bytes())
    dest = scene['tmp'] / 'never'
    with pytest.raises(ValueError, match='v_unlisted'):
        BG.extract_backgrounds([(jobs[0][0], str(dest / 'a.jpg')), (str(other), str(dest / 'b.jpg'))], method='person_masked',
                               det_file=scene['det_file'])
    assert not dest.exists()
    # frames past the end of the detection list are left out and counted
    short = dict(scene['dets'])
    short['v_moving'] = short['v_moving'][:8]                                    # entries 0..7: frames 8, 9, 10 have none
    det2 = scene['tmp'] / 'short.npy'
    np.save(det2, short, allow_pickle=True)
    report = []
    BG.extract_backgrounds([(jobs[1][0], str(tmp / 'short.jpg'))], method='person_masked', det_file=str(det2), report=report)
    assert report[0]['frames'] == 7 and report[0]['frames_without_entry'] == 3


def test_task_loop_passes_bg_extraction(dev, scene):
    import bdvcil_amd.task_loop as TL
    from test_task_loop_gpu import _config
    tmp = scene['tmp'] / 'loop'
    tmp.mkdir()
    cfg = _config(tmp, task_splits=[[0, 1]], ending_task=0, data_root=str(scene['root']))
    for name in ('train', 'val'):
        (tmp / f'{name}.txt').write_text(f'v_moving {F} 0\nv_static {F} 1\n')
    ext = dict(method='person_masked', det_file=scene['det_file'], max_hole_fraction=0.0, **DET)
    cfg['data']['train'] = dict(type='BackgroundMixDataset', bg_dir=str(tmp / 'bg'), bg_extraction=ext)
    loop = TL.CILTaskLoop(cfg, TL.SyntheticClipLoader('cuda', num_segments=8, size=32, seed=5), device='cuda', seed=0, log=lambda *a: None)
    direct = BG.resolve_bg_files(_infos(scene), str(scene['tmp'] / 'loop_direct'), bg_extraction=ext)
    assert [os.path.basename(p) for p in loop.train_dataset.bg_files] == [os.path.basename(p) for p in direct] == ['v_moving.jpg']
    assert pathlib.Path(loop.train_dataset.bg_files[0]).read_bytes() == pathlib.Path(direct[0]).read_bytes()
    assert json.loads((pathlib.Path(os.path.realpath(tmp)) / 'bg' / BG.REPORT_NAME).read_text())['videos']['v_static.jpg']['written'] is False
