"""Host side of the mixed-resolution loader: the packed layout (``RaggedLayout``), the stage planner (``plan_resize_stage``), the two
descriptor-driven entry points in header / binding / library, and their validation, which runs before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import bdvcil_amd as bd
from bdvcil_amd import decode as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bdv_resize_linear_ragged_u8', 'bdv_crop_normalize_ragged_u8')
# H x W sources: one group with scattered rows (48x64 twice, not adjacent), a wider clip, a portrait clip, a size that is no multiple
# of the MCU, an exact 2x shrink, a clip already at the short edge (copy), odd pixel counts (frames not 4-byte aligned)
SIZES = [(48, 64), (48, 88), (72, 40), (48, 64), (50, 50), (64, 96), (32, 40), (17, 23)]


def _check_layout(L, sizes, T):
    B = len(sizes)
    assert L.sizes == list(sizes) and L.T == T
    order = list(dict.fromkeys(sizes))                                   # size groups in order of first appearance
    assert L.groups == order
    assert L.rows == [[b for b in range(B) if sizes[b] == hw] for hw in order]
    for b in range(B):
        g, r = L.where[b]
        assert L.groups[g] == sizes[b] and L.rows[g][r] == b
        assert L.offsets[b] == L.group_offsets[g] + r * L.clip_stride[g]
        assert L.offsets[b] % 256 == 0                                   # every clip starts at a 256-byte boundary
        assert L.clip_bytes(b) == T * sizes[b][0] * sizes[b][1] * 3 <= L.clip_stride[g] < L.clip_bytes(b) + 256
    spans = sorted((L.offsets[b], L.offsets[b] + L.clip_bytes(b)) for b in range(B))
    assert spans[0][0] == 0 and spans[-1][1] <= L.nbytes
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))           # no two clips share a byte
    # groups are laid out back to back: group g + 1 starts where the last (padded) clip of group g ends
    assert L.group_offsets == [sum(len(L.rows[k]) * L.clip_stride[k] for k in range(g)) for g in range(len(order))]
    assert L.nbytes == sum(len(r) * s for r, s in zip(L.rows, L.clip_stride))
    assert np.array_equal(L.table(), np.array([[L.offsets[b], *sizes[b]] for b in range(B)], dtype=np.int64))


@pytest.mark.parametrize('T', [3, 8])
@pytest.mark.parametrize('sizes', [SIZES, [(48, 64)], [(48, 64), (48, 88), (48, 64), (48, 88)], SIZES[3:], [(17, 23)] * 3],
                         ids=['table', 'one_clip', 'abab', 'all_distinct', 'padded_group'])
def test_layout(sizes, T):
    _check_layout(D.RaggedLayout(sizes, T), sizes, T)


def test_layout_of_the_issue_table():
    L = D.RaggedLayout(SIZES, 3)
    assert L.rows == [[0, 3], [1], [2], [4], [5], [6], [7]] and L.where[3] == (0, 1)
    assert L.clip_stride[0] == 27648 == 3 * 48 * 64 * 3                  # a multiple of 256: the group is dense
    assert L.clip_stride[-1] == 3584 > 3 * 17 * 23 * 3 == 3519           # 17 x 23: padded up
    assert L.offsets[:4] == [0, 2 * 27648, 2 * 27648 + 38144, 27648]
    with pytest.raises(ValueError):
        D.RaggedLayout([], 3)
    with pytest.raises(ValueError):
        D.RaggedLayout([(0, 4)], 3)


def test_plan_resize_stage():
    T = 3
    src = D.RaggedLayout(SIZES, T)
    out_sizes = [D.rescale_size(w, h, (-1, 32))[::-1] for h, w in SIZES]
    assert out_sizes == [(32, 43), (32, 59), (58, 32), (32, 43), (32, 32), (32, 48), (32, 40), (32, 43)]
    dst, table = D.plan_resize_stage(src, out_sizes=out_sizes)           # Resize(-1, 32): a second packed buffer
    _check_layout(dst, out_sizes, T)
    assert dst.rows[0] == [0, 3, 7]                                      # 48x64 and 17x23 both resize to 32x43: regrouped
    assert table.dtype == np.int64 and table.shape == (8, 10)
    for b, (h, w) in enumerate(SIZES):
        assert table[b].tolist() == [src.offsets[b], h, w, 0, 0, w, h, dst.offsets[b], *out_sizes[b]]
    boxes = [(1, 2, 20, 16)] * 8
    none, table = D.plan_resize_stage(dst, boxes=boxes, uniform=(24, 24))     # MultiScaleCrop + Resize: the uniform batch, sample order
    assert none is None
    for b in range(8):
        assert table[b].tolist() == [dst.offsets[b], *out_sizes[b], 1, 2, 20, 16, b * T * 24 * 24 * 3, 24, 24]
    with pytest.raises(ValueError):
        D.plan_resize_stage(src)
    with pytest.raises(ValueError):
        D.plan_resize_stage(src, out_sizes=out_sizes, uniform=(24, 24))
    with pytest.raises(ValueError):
        D.plan_resize_stage(src, out_sizes=out_sizes[:-1])


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
        for p, a in zip(params, args):       # pointers and arrays against pointers, scalars against scalars
            assert ('*' in p or '[' in p) == (a is bd._lib.P or a is bd._lib._F3), (name, p, a)
    assert 'ragged.hip' in bd._lib.HASHED_SOURCES
    assert bd._lib.lib().bdv_abi_version() == bd._lib.ABI_VERSION == 33
    assert hasattr(bd.kernels, 'resize_linear_ragged_u8') and hasattr(bd.kernels, 'crop_normalize_ragged_u8')


# the buffers are never dereferenced: every call below fails on its table, before any launch
SRC, DST = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)


def _resize(table, src_bytes, dst_bytes, T=3):
    t = np.ascontiguousarray(table, dtype=np.int64)
    lib = bd._lib.lib()
    code = lib.bdv_resize_linear_ragged_u8(SRC, src_bytes, SRC, t.ctypes.data, len(t), T, DST, dst_bytes, None)
    return code, lib.bdv_last_error().decode()


def test_resize_validation_names_the_clip():
    T = 3
    src = D.RaggedLayout([(48, 64), (17, 23), (48, 64)], T)
    dst, good = D.plan_resize_stage(src, out_sizes=[(32, 43), (32, 43), (32, 43)])
    bad = good.copy()
    bad[1, 3:7] = (4, 0, 20, 17)                                          # x 4 + w 20 > 23
    code, msg = _resize(bad, src.nbytes, dst.nbytes)
    assert code == -1 and 'clip 1' in msg and 'leaves the 23 x 17 frame' in msg
    bad = good.copy()
    bad[2, 6] = 49                                                        # box one row taller than the frame
    code, msg = _resize(bad, src.nbytes, dst.nbytes)
    assert code == -1 and 'clip 2' in msg and 'leaves the' in msg
    code, msg = _resize(good, src.nbytes - 256, dst.nbytes)               # the last source clip (sample 1) ends past the buffer
    assert code == -1 and 'clip 1' in msg and 'source bytes' in msg and 'outside the buffer' in msg
    code, msg = _resize(good, src.nbytes, dst.offsets[2] + dst.clip_bytes(2) - 1)
    assert code == -1 and 'clip 2' in msg and 'destination bytes' in msg and 'outside the buffer' in msg
    bad = good.copy()
    bad[0, 7] = -256
    code, msg = _resize(bad, src.nbytes, dst.nbytes)
    assert code == -1 and 'clip 0' in msg and 'outside the buffer' in msg
    bad = good.copy()
    bad[2, 7] = bad[0, 7] + 16                                            # clip 2 written into the middle of clip 0
    code, msg = _resize(bad, src.nbytes, dst.nbytes)
    assert code == -1 and 'clip 2' in msg and 'overlap those of clip 0' in msg
    bad = good.copy()
    bad[1, 7] = bad[1, 7] + 8                                             # inside its padding, but not on a 16-byte boundary
    code, msg = _resize(bad, src.nbytes, dst.nbytes)
    assert code == -1 and 'clip 1' in msg and '16-byte aligned' in msg
    bad = good.copy()
    bad[2, 0] += 4
    code, msg = _resize(bad, src.nbytes + 256, dst.nbytes)
    assert code == -1 and 'clip 2' in msg and '16-byte aligned' in msg
    lib = bd._lib.lib()
    t = np.ascontiguousarray(good)
    assert lib.bdv_resize_linear_ragged_u8(SRC, src.nbytes, SRC, None, 3, T, DST, dst.nbytes, None) == -1 and b'null' in lib.bdv_last_error()
    assert lib.bdv_resize_linear_ragged_u8(SRC, src.nbytes, SRC, t.ctypes.data, 3, T, ctypes.c_void_p((1 << 20) + 4096), dst.nbytes,
                                           None) == -1 and b'overlap' in lib.bdv_last_error()


def test_crop_validation_names_the_clip():
    T = 3
    L = D.RaggedLayout([(32, 43), (58, 32), (32, 40)], T)
    clips = L.table()
    f3 = ctypes.c_float * 3
    lib = bd._lib.lib()

    def run(clips, crops, nbytes=L.nbytes, ncrops=2, ch=32, cw=32):
        c, k = np.ascontiguousarray(clips, dtype=np.int64), np.ascontiguousarray(crops, dtype=np.int32)
        code = lib.bdv_crop_normalize_ragged_u8(SRC, nbytes, SRC, c.ctypes.data, SRC, k.ctypes.data, ncrops, ch, cw, f3(0, 0, 0), f3(1, 1, 1),
                                                None, DST, len(c), T, None)
        return code, lib.bdv_last_error().decode()

    crops = np.zeros((3, 2, 3), np.int32)
    crops[0, 1] = (11, 0, 1)
    crops[1, 1] = (0, 26, 0)
    crops[2, 1] = (9, 0, 0)                                               # 9 + 32 > 40
    code, msg = run(clips, crops)
    assert code == -1 and 'clip 2' in msg and 'crop 1 at (9, 0) leaves the 32x40 frame' in msg
    crops[2, 1] = (8, 0, 0)
    code, msg = run(clips, crops, nbytes=L.offsets[1] + L.clip_bytes(1) - 1)
    assert code == -1 and 'clip 1' in msg and 'outside the buffer' in msg
    code, msg = run(clips, crops, ch=33)
    assert code == -1 and 'clip 0' in msg and '33x32 crop of 32x43' in msg
    code, msg = run(clips, np.zeros((3, 13, 3), np.int32), ncrops=13)
    assert code == -1 and '13 crops' in msg
