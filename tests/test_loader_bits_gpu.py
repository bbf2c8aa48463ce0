"""The loader kernels' output BITS at small shapes, against hashes recorded before their shared pieces were given one definition each
(csrc/resize_linear.h, csrc/loader_pieces.h, csrc/common.h; the ``bits`` section of tests/golden/loader_bits.json -- ``python
tests/test_loader_bits_gpu.py`` on a GPU re-records it from the library ``BDVCIL_LIB_PATH`` names).  The other loader suites allow
tolerances or compare against a CPU restatement; this one holds the outputs to what the library computed before, bit for bit.  Every call
goes through the Python bindings; inputs are seeded on the CPU.  Each shape is the smallest at which its path can go wrong:

  resize_linear_u8          5x7 -> 5x7 (copy, 35 pixels: byte tail); 8x12 -> 4x6 (2x mean, whole dwords); 9x13 -> 6x10 (resample, whole
                            dwords); 9x13 -> 5x7 (resample, tail); (B 2, T 2) with boxes (1,2,8,6) and (0,0,13,9) -> 3x4 and -> 5x7
  resize_linear_ragged_u8   clips 6x9, 8x8, 5x12 of T 2: a copy, a 2x mean and a resample to 36x32 (a second block column) in one
                            launch; then 6x9 -> 4x6 (its blocks beyond the frame exit) beside the 36x32 one and a box that is copied
  crop_normalize_u8         B 2, T 2, 9x11, crop 5x6 at (0,0), (5,4) flipped, (2,1); both outputs, NHWC4 only, NCHW only
  crop_normalize_ragged_u8  clips 9x11 and 7x13, the same crop size, per-clip crops with flips
  bgmix_normalize_u8        B 2, T 3, 5x7, mix [1, 0], uint8 and fp32 background (the kernel of the benchmarked step)
  actor_cut_mix_u8          T 2, actor 10x14 -> 5x7 (2x, odd pixel count) and -> 6x10 (resample, wide store), scene 9x13; actor and scene
                            flips, a cut-out box, one clip without actor boxes (scene row -1); the counts are hashed too
  blend_mix                 B 3, S 210 and S 7, perm [2, 0, 1]
  blend_box_                B 3, outer 2, 6x7, inner 1 and 4, rows 1:2 cols 4:6, a perm with a fixed point
  fg_motion_q .. fg_merge_  B 3, T 3, 9x11 (odd H * W) in the three layouts; perm [1, 2, 2] with apply [1, 1, 0]: clip 0 takes from
                            clip 1, which is itself merged (the staged path)
  temporal_median_u8, temporal_masked_median_u8, temporal_nanreduce_f32 (median and mean)
                            counts [1, 2, 5] at 3x5 (45 bytes per frame: unaligned) and 4x4 (aligned)"""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loader_bits.json')
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

CASES = [('resize', 'copy'), ('resize', 'half'), ('resize', 'resample_dwords'), ('resize', 'resample_tail'), ('resize', 'boxes_3x4'),
         ('resize', 'boxes_5x7'), ('resize_ragged', 'three_paths'), ('resize_ragged', 'block_columns'), ('crop', 'both'), ('crop', 'nhwc4'),
         ('crop', 'nchw'), ('crop_ragged', 'both'), ('bgmix', 'u8'), ('bgmix', 'f32'), ('acm', '5x7'), ('acm', '6x10'), ('blend_mix', 210),
         ('blend_mix', 7), ('blend_box', 1), ('blend_box', 4), ('fg', 'tchw'), ('fg', 'cthw'), ('fg', 'thwc4'), ('temporal', '3x5'),
         ('temporal', '4x4')]


def _key(case):
    return '/'.join(map(str, case))


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.uint16 else t).numpy().tobytes()).hexdigest()


def _pair(o4, oc):
    return {n: _sha(t) for n, t in (('nhwc4', o4), ('nchw', oc)) if t is not None}


def loader_hashes(case, dev):
    import bdvcil_amd as bd
    from bdvcil_amd import decode as D
    from bdvcil_amd import kernels as K
    from bdvcil_amd.actor_cut_mix import acm_plan_table
    gen = torch.Generator().manual_seed(9000 + CASES.index(case))
    u8 = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, generator=gen)              # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=gen)                                          # noqa: E731
    kind, what = case
    out = {}
    if kind == 'resize':
        src, dst, boxes = {'copy': ((2, 5, 7), (5, 7), None), 'half': ((2, 8, 12), (4, 6), None), 'resample_dwords': ((2, 9, 13), (6, 10), None),
                           'resample_tail': ((2, 9, 13), (5, 7), None), 'boxes_3x4': ((2, 2, 9, 13), (3, 4), [(1, 2, 8, 6), (0, 0, 13, 9)]),
                           'boxes_5x7': ((2, 2, 9, 13), (5, 7), [(1, 2, 8, 6), (0, 0, 13, 9)])}[what]
        out = dict(out=_sha(K.resize_linear_u8(u8(*src, 3).to(dev), dst[0], dst[1], boxes=boxes)))
    elif kind == 'resize_ragged':
        T = 2
        src = D.RaggedLayout([(6, 9), (8, 8), (5, 12)], T)
        sizes = [(6, 9), (4, 4), (36, 32)] if what == 'three_paths' else [(4, 6), (4, 4), (36, 32)]
        dst, table = D.plan_resize_stage(src, out_sizes=sizes)
        if what == 'block_columns':
            table[1, 3:7] = (2, 3, 4, 4)                                                    # a 4x4 box of the 8x8 clip: copied
        buf = torch.zeros(dst.nbytes, dtype=torch.uint8, device=dev)                        # the padding between clips stays 0
        out = dict(out=_sha(K.resize_linear_ragged_u8(u8(src.nbytes).to(dev), table, T, buf)))
    elif kind == 'crop':
        o4, oc = K.crop_normalize_u8(u8(2, 2, 9, 11, 3).to(dev), [(0, 0, 0), (5, 4, 1), (2, 1, 0)], 5, 6, MEAN, STD,
                                     want_nhwc4=what != 'nchw', want_nchw=what != 'nhwc4')
        out = _pair(o4, oc)
        assert set(out) == {'both': {'nhwc4', 'nchw'}, 'nhwc4': {'nhwc4'}, 'nchw': {'nchw'}}[what]
    elif kind == 'crop_ragged':
        L = D.RaggedLayout([(9, 11), (7, 13)], 2)
        crops = [[(0, 0, 0), (5, 4, 1), (2, 1, 0)], [(7, 2, 1), (0, 0, 0), (3, 1, 1)]]
        out = _pair(*K.crop_normalize_ragged_u8(u8(L.nbytes).to(dev), L.table(), 2, crops, 5, 6, MEAN, STD, want_nhwc4=True, want_nchw=True))
    elif kind == 'bgmix':
        frames, bg = u8(2, 3, 5, 7, 3), u8(2, 5, 7, 3)
        if what == 'f32':
            bg = bg.float() + torch.rand(2, 5, 7, 3, generator=gen) * 0.99
        out = _pair(*K.bgmix_normalize_u8(frames.to(dev), bg.to(dev), torch.tensor([1, 0], dtype=torch.uint8).to(dev), 0.5, MEAN, STD,
                                          want_nhwc4=True, want_nchw=True))
    elif kind == 'acm':
        Hd, Wd = (5, 7) if what == '5x7' else (6, 10)
        actor, scene = u8(2, 2, 10, 14, 3), u8(2, 2, 9, 13, 3)
        clips = [(1, 0, 1, 1, 0), (0, 1, 0, 0, 1), (2, 0, 0, -1, 0)]       # (out row, actor row, actor flip, scene row, scene flip)
        actor_boxes = [[[(1, 1, 5, 4)], [(0, 0, 3, 2), (4, 2, 7, 5)]], [[(2, 0, 6, 5)], []], [[], []]]
        scene_boxes = [[[(5, 0, 7, 2)], []], [[], [(0, 3, 2, 5)]], [[], []]]
        res = torch.zeros(3, 2, 3, Hd, Wd, dtype=torch.float32, device=dev)
        counts = K.actor_cut_mix_u8(actor.to(dev), scene.to(dev), acm_plan_table(clips, actor_boxes, scene_boxes), 3, res, MEAN, STD)
        out = dict(out=_sha(res), counts=_sha(counts))
    elif kind == 'blend_mix':
        out = dict(out=_sha(K.blend_mix(rn(3, what).to(dev), torch.tensor([2, 0, 1]), 0.3)))
    elif kind == 'blend_box':
        x = rn(3, 2, 6, 7, what).to(dev) if what == 4 else rn(3, 2, 6, 7).to(dev)
        out = dict(out=_sha(K.blend_box_(x, torch.tensor([1, 0, 2]), (1, 4, 2, 6), 2, 6, 7, inner=what)))
    elif kind == 'fg':
        B, T, H, W = 3, 3, 9, 11
        x = rn(*{'tchw': (B, T, 3, H, W), 'cthw': (B, 3, T, H, W), 'thwc4': (B * T, H, W, 4)}[what]).to(dev)
        q, g, d = K.fg_motion_q(x, B, T, H, W, layout=what)
        lo, scale = K.fg_colour_params(8, MEAN, STD)
        s, F, N = K.fg_hist_refine(x, q, B, T, H, W, layout=what, bins=8, lo=lo, scale=scale)
        v, mask, count = K.fg_select(s, K.fg_k_fg(0.3, H, W))
        merged = K.fg_merge_(x.clone(), mask, count, torch.tensor([1, 2, 2]), torch.tensor([True, True, False]), B, T, H, W, layout=what)
        out = {n: _sha(t) for n, t in dict(q=q, g=g, d=d, s=s, F=F, N=N, v=v, mask=mask, count=count, merged=merged).items()}
        assert int(count[1]) > 0 and not torch.equal(merged, x)               # clip 1 is merged, so clip 0's source is staged
    else:
        assert kind == 'temporal'
        H, W = (3, 5) if what == '3x5' else (4, 4)
        counts = [1, 2, 5]
        frames = u8(8, H, W, 3)
        med = bd.background.temporal_median(frames.to(dev), counts)
        box_first = [0, 0, 1, 1, 2, 2, 2, 3, 3]
        boxes = [(0, 0, 2, 2), (1, 1, W, H), (0, 1, 3, 3)]
        masked, visible = K.temporal_masked_median_u8(frames.to(dev), counts, box_first, boxes, min_visible=1)
        f = u8(8, H, W, 3).float()
        hole = torch.rand(8, H, W, 3, generator=gen)
        f[hole < 0.2] = 0.0
        f[hole > 0.9] = float('nan')
        out = dict(median=_sha(med), masked=_sha(masked), visible=_sha(visible),
                   nanmedian=_sha(K.temporal_nanreduce_f32(f.to(dev), counts, mode=0)), nanmean=_sha(K.temporal_nanreduce_f32(f.to(dev), counts, mode=1)))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)['bits']


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(_key(c) for c in CASES) and len({_key(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=_key)
def test_loader_output_bits(case, golden, dev):
    assert loader_hashes(case, dev) == golden[_key(case)]


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        with open(GOLDEN) as f:
            table = json.load(f)
    except FileNotFoundError:
        table = {}
    table['bits'] = {_key(c): loader_hashes(c, torch.device('cuda:0')) for c in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', len(table['bits']), 'cases')
