"""ActorCutMix on the host, against tests/golden/actor_cut_mix_golden.npz (the reference's own box.py / actor_cut_mix_loader.py,
make_golden_actor_cut_mix.py): the box chain, a numpy restatement of the mask + composite + ratio, the order of ``draw()``'s random
draws, and the detection-key rules.  No GPU."""
import os
import random

import numpy as np
import pytest

from oracle import resize_oracle as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'actor_cut_mix_golden.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD, allow_pickle=False))


def fixture_videos(g):
    """(video_infos, detections dict keyed by video name, frames per frame_dir) of the fixture."""
    infos, dets, frames = [], {}, {}
    for k in range(int(g['n_videos'])):
        fd = str(g[f'v{k}_frame_dir'])
        infos.append(dict(frame_dir=fd, total_frames=int(g[f'v{k}_total']), label=int(g[f'v{k}_label'])))
        dets[fd.split('/')[-1]] = [g[f'v{k}_det{i}'] for i in range(int(g[f'v{k}_ndet']))]
        frames[fd] = g[f'v{k}_frames']
    return infos, dets, frames


def human_mask(boxes, H, W):
    """BuildHumanMask (box.py:176-207) for one clip of int boxes: (T, H, W) uint8; all ones when the clip has no box."""
    T = len(boxes)
    if sum(len(b) for b in boxes) == 0:
        return np.ones((T, H, W), np.uint8)
    m = np.zeros((T, H, W), np.uint8)
    for t, bs in enumerate(boxes):
        for b in bs:
            m[t, b[1]:b[3], b[0]:b[2]] = 1
    return m


def composite(actor, scene, aboxes, sboxes):
    """actor / scene (T, H, W, 3) uint8 after flip + resize -> (composite uint8, mask (T, H, W)): ActorCutOut(127) of the scene,
    actor * mask + scene * (1 - mask) (actor_cut_mix_loader.py:143-149).  SceneCutOut never reaches the output."""
    T, H, W, _ = actor.shape
    mask = human_mask(aboxes, H, W)
    scene = scene.copy()
    if sum(len(b) for b in sboxes):
        for t, bs in enumerate(sboxes):
            for b in bs:
                scene[t, b[1]:b[3], b[0]:b[2]] = 127
    m3 = mask[..., None]
    return actor * m3 + scene * (1 - m3), mask


def flip_resize(frames, short, out_hw, flip):
    """decode -> Resize(-1, short) -> optional horizontal flip -> Resize((out_hw, out_hw)) on the CPU (resize oracle)."""
    out = []
    for f in frames:
        Wr, Hr = R.rescale_size(f.shape[1], f.shape[0], (-1, short))
        r = R.resize_linear_u8(f, Wr, Hr)
        if flip:
            r = np.ascontiguousarray(np.flip(r, 1))
        out.append(R.resize_linear_u8(r, out_hw, out_hw))
    return np.stack(out)


def test_box_chain_and_composite_equal_the_reference(gold):
    from bdvcil_amd.actor_cut_mix import clip_boxes, detection_load, flip_boxes, resize_boxes
    g = gold
    infos, dets, frames = fixture_videos(g)
    T, short, S, thres = int(g['T']), int(g['short']), int(g['out_hw']), float(g['thres'])
    kinds = set()
    for s in range(int(g['n_samples'])):
        p = f's{s}_'
        a, sc = infos[int(g[p + 'actor'])], infos[int(g[p + 'scene'])]
        clips = []
        for v, inds, flip, tag in ((a, g[p + 'actor_inds'], bool(g[p + 'actor_flip']), 'abox'),
                                   (sc, g[p + 'scene_inds'], bool(g[p + 'scene_flip']), 'sbox')):
            H0, W0 = frames[v['frame_dir']].shape[1:3]
            all_dets = dets[v['frame_dir'].split('/')[-1]]
            # the float boxes, step by step, in the detection array's own dtype
            fl = detection_load(all_dets, inds, thres)
            w1, h1 = R.rescale_size(W0, H0, (-1, short))
            resize_boxes(fl, W0, H0, w1, h1)
            if flip:
                fl = flip_boxes(fl, w1)
            resize_boxes(fl, w1, h1, S, S)
            for t in range(T):
                want = g[p + f'{tag}{t}']
                assert fl[t].dtype == want.dtype and np.array_equal(fl[t], want), (s, tag, t)
            ib = clip_boxes(all_dets, inds, W0, H0, short, S, S, flip, thres)
            assert all(np.array_equal(x, w.astype(int)) for x, w in zip(ib, (g[p + f'{tag}{t}'] for t in range(T))))
            clips.append((flip_resize(frames[v['frame_dir']][inds], short, S, flip), ib))
        (actor, ab), (scene, sb) = clips
        img, mask = composite(actor, scene, ab, sb)
        assert np.array_equal(mask, g[p + 'mask']), s
        assert np.array_equal(img, g[p + 'imgs']), s
        ratio = mask.astype(np.int64).sum() / (T * S * S)
        assert ratio == float(g[p + 'ratio']) and int(g[p + 'bg_label']) == sc['label']
        nb = [len(b) for b in ab]
        kinds.add('none' if sum(nb) == 0 else 'some' if min(nb) == 0 else 'all')
        kinds.add(('flip', bool(g[p + 'actor_flip']), bool(g[p + 'scene_flip'])))
    assert {'none', 'some', 'all'} <= kinds and sum(1 for k in kinds if isinstance(k, tuple)) == 4


def _loader(tmp_path, dets, **kw):
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    path = tmp_path / kw.pop('det_name', 'detections.npy')
    np.save(path, np.array(dets, dtype=object), allow_pickle=True)
    return ActorCutMixClipLoader(str(path), device='cpu', num_segments=4, short_edge=40, input_size=32, **kw)


def test_draw_consumes_the_generators_in_the_reference_order(gold, tmp_path):
    g = gold
    infos, dets, frames = fixture_videos(g)
    loader = _loader(tmp_path, dets, acm_prob=0.5)
    loader.set_scene_infos(infos)
    random.seed(int(g['seq_seed']))
    np.random.seed(int(g['seq_seed']))
    for n, idx in enumerate(g['seq_order'].tolist()):
        H0, W0 = frames[infos[idx]['frame_dir']].shape[1:3]
        Wr, Hr = R.rescale_size(W0, H0, (-1, 40))
        plan = loader.draw([infos[idx]], (Hr, Wr))        # one sample at a time: the fixture's videos differ in size
        r, ex = plan.rows[0], g['seq_extra'][n].tolist()
        assert r.acm == bool(g['seq_acm'][n]), n
        assert r.frame_inds.tolist() == g['seq_inds'][n].tolist(), n
        if r.acm:
            assert [int(r.flip), r.scene_index, int(r.scene_flip)] == ex[:3], n
            assert r.scene_inds.tolist() == g[f'seq{n}_scene_inds'].tolist(), n
        else:
            assert list(r.crop) == ex[1:], n
    assert random.random() == float(g['seq_next_random']) and np.random.rand() == float(g['seq_next_np'])
    assert 0 < int(g['seq_acm'].sum()) < len(g['seq_acm'])


def test_detection_keys(tmp_path):
    from bdvcil_amd.actor_cut_mix import detection_key
    assert detection_key('/data/ucf101/rawframes/ApplyEyeMakeup/v_ApplyEyeMakeup_g08_c01', '/data/ucf101/detections.npy') == \
        'v_ApplyEyeMakeup_g08_c01'
    assert detection_key('/data/kinetics400/rawframes_train/abseiling/0347ZoDXyP0_000095_000105',
                         '/data/kinetics400/detections.npy') == '0347ZoDXyP0'
    # the rule follows the detection file's path, as load_detections does
    assert detection_key('/data/kinetics400/x/0347ZoDXyP0_000095_000105', '/data/ucf101/detections.npy') == '0347ZoDXyP0_000095_000105'
    box = np.array([[1.0, 2.0, 3.0, 4.0, 0.9]], np.float32)
    loader = _loader(tmp_path, {'v_a': [box] * 3, '0347ZoDXyP0': [box] * 3}, det_name='kinetics_detections.npy')
    assert loader.video_detections({'frame_dir': '/k/abseiling/0347ZoDXyP0_000095_000105'})[0] is not None
    loader.set_scene_infos([{'frame_dir': '/k/v_a', 'total_frames': 2, 'label': 0}])         # 'v_a'[:11] == 'v_a': found
    assert loader.scene_infos == [{'frame_dir': '/k/v_a', 'total_frames': 2, 'label': 0}]
    with pytest.raises(KeyError):
        loader.set_scene_infos([{'frame_dir': '/k/missing_video_x', 'total_frames': 2, 'label': 0}])


def test_detection_load_quirks():
    from bdvcil_amd.actor_cut_mix import detection_load
    per = [np.array([[0, 0, 1, 1, 0.9]], np.float64), np.array([[1, 1, 2, 2, 0.4], [2, 2, 3, 3, 0.41]], np.float64)]
    out = detection_load(per, np.array([1]))             # frame number 1 reads entry 1 (the 1-based quirk)
    assert out[0].tolist() == [[2, 2, 3, 3]]             # strict threshold: the 0.4 row is dropped
    with pytest.raises(IndexError):
        detection_load(per, np.array([2]))
