"""Every refusal of the loader entry points whose host code was folded onto shared helpers (csrc/common.h: the video-run validator and
the grid helper; csrc/loader_pieces.h: the Normalize parameters): the (return code, bdv_last_error() text) of each branch against the
``refusals`` section of tests/golden/loader_bits.json, recorded from the library before the fold (``python
tests/test_loader_refusals_cpu.py`` re-records the section from the library ``BDVCIL_LIB_PATH`` names).  A refusal comes before any
launch: the buffers below are addresses that are never dereferenced, and no GPU is needed.

  bdv_temporal_median_u8, bdv_temporal_masked_median_u8, bdv_temporal_nanreduce_f32
                                  the (first, counts) table: a video of 0 / 65536 frames, a negative first frame, a run past the end,
                                  each in a video that is not the first
  bdv_crop_normalize_u8           null pointer, no output, 0 / 13 crops, crop larger than the frame, misaligned NHWC4 output, a crop
                                  that leaves the frame on each of its four sides
  bdv_crop_normalize_ragged_u8    the same, and per clip: bad frame size, crop larger than the clip's frame, bytes outside the buffer
  bdv_resize_linear_u8            null / in-place, bad shape, boxes on one side only, frames that are not whole groups, a box that
                                  leaves the frame, too many frames, misaligned destination
  bdv_resize_linear_ragged_u8     null, bad shape, overlapping buffers, misaligned buffers, and per clip: bad frame size, box, clip
                                  alignment, source / destination bytes outside, overlapping destinations

Also here: BackgroundCropFrontEnd refuses crop offsets outside the resized image before it touches the device."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'loader_bits.json')
A, B_, C = 1 << 20, 1 << 24, 1 << 26          # three "buffers", 16-byte aligned, far apart
F3 = ctypes.c_float * 3
MEAN, INV = F3(0, 0, 0), F3(1, 1, 1)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def _runs(first, counts):
    return _i64(first), _i32(counts)


# (first, counts) of three videos in 8 frames; video 1 or 2 is wrong
BAD_RUNS = {
    'no_frames': ([0, 1, 1], [1, 0, 7]),
    'too_many_frames': ([0, 1, 3], [1, 2, 65536]),
    'negative_first': ([0, -1, 3], [1, 2, 5]),
    'past_the_end': ([0, 1, 3], [1, 2, 6]),
}


def _median(lib, first, counts):
    f, c = _runs(first, counts)
    return lib.bdv_temporal_median_u8(A, 8, A, A, f.ctypes.data, c.ctypes.data, 3, 3, 5, B_, None)


def _masked_median(lib, first, counts):
    f, c = _runs(first, counts)
    bf = _i32([0] * 9)
    return lib.bdv_temporal_masked_median_u8(A, 8, A, A, f.ctypes.data, c.ctypes.data, 3, 3, 5, A, None, bf.ctypes.data, None, 0, 1, B_, C, None)


def _nanreduce(lib, first, counts):
    f, c = _runs(first, counts)
    return lib.bdv_temporal_nanreduce_f32(A, 8, A, A, f.ctypes.data, c.ctypes.data, 3, 15, 0, 1, B_, None)


def _crop(lib, frames=A, crops=((0, 0, 0), (5, 4, 1)), ncrops=None, ch=5, cw=6, o4=B_, oc=C, H=9, W=11):
    t = _i32(crops)
    return lib.bdv_crop_normalize_u8(frames, t.ctypes.data, len(t) if ncrops is None else ncrops, ch, cw, MEAN, INV, o4, oc, 2, 2, H, W, None)


RAG_CLIPS = [(0, 9, 11), (2 * 9 * 11 * 3 + 6, 7, 13)]          # (byte offset, H, W) of two clips of T = 2 frames; 600 = 594 + 6
RAG_BYTES = 600 + 2 * 7 * 13 * 3
RAG_CROPS = [[(0, 0, 0), (5, 4, 1)], [(7, 2, 1), (0, 0, 0)]]


def _crop_ragged(lib, src=A, clips=RAG_CLIPS, crops=RAG_CROPS, nbytes=RAG_BYTES, ncrops=2, ch=5, cw=6, o4=B_, oc=C, clips_host=True):
    c, k = _i64(clips), _i32(crops)
    return lib.bdv_crop_normalize_ragged_u8(src, nbytes, A, c.ctypes.data if clips_host else None, A, k.ctypes.data, ncrops, ch, cw, MEAN, INV,
                                            o4, oc, len(c), 2, None)


def _resize(lib, src=A, N=4, Hs=9, Ws=13, boxes=None, dev_boxes='same', per=2, dst=B_, Hd=5, Wd=7):
    hb = None if boxes is None else _i32(boxes)
    dev = (None if hb is None else A) if dev_boxes == 'same' else dev_boxes
    return lib.bdv_resize_linear_u8(src, N, Hs, Ws, dev, per, None if hb is None else hb.ctypes.data, dst, Hd, Wd, None)


# rows (source byte, Hs, Ws, x0, y0, w, h, destination byte, Hd, Wd) of two clips of T = 2 frames
RS_TABLE = [[0, 6, 9, 0, 0, 9, 6, 0, 6, 9], [336, 8, 8, 0, 0, 8, 8, 336, 4, 4]]
RS_SRC, RS_DST = 336 + 2 * 8 * 8 * 3, 336 + 2 * 4 * 4 * 3


def _resize_ragged(lib, table=RS_TABLE, edit=None, src=A, dst=B_, src_bytes=RS_SRC, dst_bytes=RS_DST, T=2, host=True):
    t = _i64(table).copy()
    for (r, c), v in (edit or {}).items():
        t[r, c] = v
    return lib.bdv_resize_linear_ragged_u8(src, src_bytes, A, t.ctypes.data if host else None, len(t), T, dst, dst_bytes, None)


def _cases():
    c = {}
    for name, (first, counts) in BAD_RUNS.items():
        c['temporal_median_u8/' + name] = lambda lib, a=(first, counts): _median(lib, *a)
        c['temporal_masked_median_u8/' + name] = lambda lib, a=(first, counts): _masked_median(lib, *a)
        c['temporal_nanreduce_f32/' + name] = lambda lib, a=(first, counts): _nanreduce(lib, *a)
    crop = {
        'null': dict(frames=None), 'no_output': dict(o4=None, oc=None), 'no_crops': dict(ncrops=0), 'too_many_crops': dict(crops=[(0, 0, 0)] * 13),
        'crop_taller': dict(ch=10), 'crop_wider': dict(cw=12), 'nhwc4_misaligned': dict(o4=B_ + 4), 'left': dict(crops=[(0, 0, 0), (-1, 0, 0)]),
        'above': dict(crops=[(0, -1, 0)]), 'right': dict(crops=[(0, 0, 0), (6, 4, 1)]), 'below': dict(crops=[(5, 5, 0)]),
    }
    for name, kw in crop.items():
        c['crop_normalize_u8/' + name] = lambda lib, kw=kw: _crop(lib, **kw)
    ragged = {
        'null': dict(src=None), 'null_host_table': dict(clips_host=False), 'no_output': dict(o4=None, oc=None), 'no_crops': dict(ncrops=0),
        'too_many_crops': dict(ncrops=13), 'bad_shape': dict(ch=0), 'nhwc4_misaligned': dict(o4=B_ + 8),
        'clip_frame_size': dict(clips=[RAG_CLIPS[0], (600, 7, 1 << 15)]), 'clip_smaller_than_crop': dict(clips=[RAG_CLIPS[0], (600, 4, 13)]),
        'clip_negative_offset': dict(clips=[(-16, 9, 11), RAG_CLIPS[1]]), 'clip_past_the_end': dict(nbytes=RAG_BYTES - 1),
        'left': dict(crops=[RAG_CROPS[0], [(-1, 0, 0), (0, 0, 0)]]), 'right': dict(crops=[RAG_CROPS[0], [(8, 2, 1), (0, 0, 0)]]),
        'below': dict(crops=[[(0, 0, 0), (5, 5, 1)], RAG_CROPS[1]]),
    }
    for name, kw in ragged.items():
        c['crop_normalize_ragged_u8/' + name] = lambda lib, kw=kw: _crop_ragged(lib, **kw)
    resize = {
        'null': dict(src=None), 'in_place': dict(dst=A), 'bad_shape': dict(Hd=0), 'boxes_host_only': dict(boxes=[(0, 0, 13, 9)] * 2, dev_boxes=None),
        'boxes_device_only': dict(dev_boxes=A), 'not_whole_groups': dict(boxes=[(0, 0, 13, 9)], per=3), 'no_frames_per_box': dict(boxes=[(0, 0, 13, 9)], per=0),
        'box_right': dict(boxes=[(0, 0, 13, 9), (6, 0, 8, 9)]), 'box_below': dict(boxes=[(0, 2, 13, 8), (0, 0, 13, 9)]),
        'box_empty': dict(boxes=[(0, 0, 13, 9), (0, 0, 0, 9)]), 'box_negative': dict(boxes=[(-1, 0, 13, 9), (0, 0, 13, 9)]),
        'too_many_frames': dict(N=65536), 'frame_too_large': dict(Hs=1 << 15, Ws=1 << 14), 'dst_misaligned': dict(dst=B_ + 2),
    }
    for name, kw in resize.items():
        c['resize_linear_u8/' + name] = lambda lib, kw=kw: _resize(lib, **kw)
    rr = {
        'null': dict(src=None), 'null_host_table': dict(host=False), 'bad_shape': dict(T=0), 'too_many_frames': dict(T=32768),
        'buffers_overlap': dict(dst=A + 64), 'buffers_misaligned': dict(src=A + 8), 'clip_frame_size': dict(edit={(1, 2): 0}),
        'clip_dst_size': dict(edit={(0, 8): 1 << 15}), 'box_right': dict(edit={(1, 3): 1}), 'box_empty': dict(edit={(0, 6): 0}),
        'clip_src_misaligned': dict(edit={(1, 0): 328}), 'clip_dst_misaligned': dict(edit={(1, 7): 340}), 'src_negative': dict(edit={(0, 0): -16}),
        'src_past_the_end': dict(src_bytes=RS_SRC - 1), 'dst_negative': dict(edit={(0, 7): -16}), 'dst_past_the_end': dict(dst_bytes=RS_DST - 1),
        'dst_overlap': dict(edit={(1, 7): 320}),
    }
    for name, kw in rr.items():
        c['resize_linear_ragged_u8/' + name] = lambda lib, kw=kw: _resize_ragged(lib, **kw)
    return c


CASES = _cases()


def _refusal(name):
    import bdvcil_amd as bd
    lib = bd._lib.lib()
    code = CASES[name](lib)
    return [code, lib.bdv_last_error().decode()]


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)['refusals']


def test_golden_holds_exactly_these_refusals(golden):
    assert sorted(golden) == sorted(CASES)
    assert all(code != 0 and text for code, text in golden.values())
    assert len({text for _, text in golden.values()}) > len(golden) // 2          # the branches are told apart by their text


@pytest.mark.parametrize('name', sorted(CASES))
def test_refusal_code_and_message(name, golden):
    assert _refusal(name) == golden[name]


def test_background_crop_offsets_are_checked_before_the_device():
    import torch
    from bdvcil_amd.frontend import BackgroundCropFrontEnd
    fe = BackgroundCropFrontEnd(8, (6, 7))                       # 6 x 9 images resize to 8 x 12: 0 <= top <= 2, 0 <= left <= 5
    bg = torch.zeros(2, 6, 9, 3, dtype=torch.uint8)              # on the CPU: any device call would fail on it with another error
    for tops, lefts in (([0, 3], [0, 0]), ([-1, 0], [0, 0]), ([0, 0], [5, 6]), ([0, 0], [0, -1])):
        with pytest.raises(ValueError, match='must lie inside the resized 8x12 image'):
            fe(bg, offsets=(tops, lefts))
    for tops, lefts in (([0], [0]), ([0, 0], [0, 0, 0])):
        with pytest.raises(ValueError, match='for 2 images'):
            fe(bg, offsets=(tops, lefts))
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):               # the corners pass and reach the binding's tensor checks
        fe(bg, offsets=([0, 2], [5, 0]))
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):               # a crop larger than the image is the binding's to refuse
        BackgroundCropFrontEnd(5, (6, 7))(bg, offsets=([9, 9], [9, 9]))


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    try:
        with open(GOLDEN) as f:
            table = json.load(f)
    except FileNotFoundError:
        table = {}
    table['refusals'] = {name: _refusal(name) for name in sorted(CASES)}
    with open(GOLDEN, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', len(table['refusals']), 'refusals')
