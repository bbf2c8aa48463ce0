"""The conv kernels' output BITS at small shapes, against hashes recorded before the dispatch went through one planner
(tests/golden/conv_bits.json; ``python tests/test_conv_bits_gpu.py`` on a GPU re-records them).  A convolution that is routed to
another kernel, another tile or another K-split sums in another order and changes the hash; parity with the CPU oracle is the
business of the other conv suites.  Inputs are seeded on the CPU.  Each shape is the smallest with a full and a partial row tile.

A second list (tests/golden/conv_bits_launch.json, recorded before the launch layer was rewritten; ``python
tests/test_conv_bits_gpu.py launch`` re-records it) runs what the first leaves out and a wrong instantiation would change: the
'f16x2' arithmetic, bf16 storage, the eval-mode BatchNorm epilogue, the producer's BatchNorm in the fprop and wgrad loaders, the ReLU
sign derived from y in the dgrad statistics, the small weight-gradient tile forms with and without the two-stage loop, and the
remaining (arithmetic, tile) pairs of the plane kernels; tests/test_conv_launch_cpu.py checks that the two lists together plan every
kernel name of tests/golden/conv_plan_sites.json.  Its last seven cases take each kernel family through what its tile prologue and
K-step state decide: a stride-2 site of odd size (unequal parity classes, blocks of the padded grid that exit), a ragged last row
tile, K-split remainder tiles with the fix-up launch, the temporal shift, and the stem's temporal taps."""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_bits.json')

# (N, H, W, Cin, Cout, R, stride, pad, T, fold)
SHAPES = [
    (3, 14, 14, 128, 128, 3, 1, 1, 1, 0),
    (3, 14, 14, 256, 64, 1, 1, 0, 3, 32),       # 1x1 with the temporal shift
    (2, 28, 28, 64, 64, 3, 1, 1, 1, 0),
    (3, 15, 15, 128, 128, 3, 2, 1, 1, 0),       # stride 2 on an odd size: unequal parity classes
    (2, 14, 14, 512, 1024, 1, 2, 0, 1, 0),
    (4, 7, 7, 512, 2048, 1, 1, 0, 1, 0),
    (2, 32, 32, 4, 64, 7, 2, 3, 1, 0),          # the stem: fprop and wgrad only
]
PL_TILE_BN = (256, 128, 256, 64, 128, 128)      # column counts of the forced tiles 0..5

# (shape index, arithmetic, forced tile)
PARAMS = [(i, mode, -1) for i in range(len(SHAPES)) for mode in ('bf16x3', 'f32mfma')]
PARAMS += [(i, mode, -1) for i in (0, 1) for mode in ('bf16x1', 'bf16x2')]
PARAMS += [(0, 'bf16x3', t) for t in range(6) if SHAPES[0][4] % PL_TILE_BN[t] == 0]

# ---- the second list ----
GOLDEN_LAUNCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_bits_launch.json')
# 1x1 sites of the weight-gradient tile forms the shapes above do not reach (64 x 64, 256 x 64, 256 x 128, 128 x 256)
WGRAD_SHAPES = [
    (2, 14, 14, 64, 64, 1, 1, 0, 1, 0),
    (2, 14, 14, 64, 256, 1, 1, 0, 1, 0),
    (2, 14, 14, 128, 256, 1, 1, 0, 1, 0),
    (2, 14, 14, 256, 128, 1, 1, 0, 1, 0),
]
# what the shapes above leave out of the tile prologues: a 3x3 site with the temporal shift and a K long enough for a K split, and the
# stem on an odd size (a ragged last row tile), without and with temporal taps (two more fields: Rt, st_t; N = output frames)
PROLOGUE_SHAPES = [
    (2, 9, 9, 128, 128, 3, 1, 1, 2, 16),
    (2, 13, 13, 4, 64, 7, 2, 3, 1, 0),
    (4, 13, 13, 4, 64, 7, 2, 3, 2, 0, 3, 2),
]
ALL_SHAPES = SHAPES + WGRAD_SHAPES + PROLOGUE_SHAPES
NEW = tuple(range(len(SHAPES), len(SHAPES) + len(WGRAD_SHAPES)))
PRO = tuple(range(len(SHAPES) + len(WGRAD_SHAPES), len(ALL_SHAPES)))
# (shape index, arithmetic, forced tile, variant).  Variants: 'plain' = the calls of the first list; 'onestage' = the same with
# BDVCIL_WGRAD_2STAGE=0; 'affine' = conv_fprop(affine=(scale, shift, residual, True)); 'pre_bn' = conv_fprop / conv_wgrad with the
# producer's BatchNorm in the loader; 'relu_affine' = conv_dgrad with the 5-tuple bn_stats (ReLU sign derived from y)
LAUNCH_PARAMS = [(i, 'f16x2', -1, 'plain') for i in (0, 1, 2)] + [(i, 'bf16', -1, 'plain') for i in (0, 2)]
LAUNCH_PARAMS += [(0, 'bf16x3', -1, 'affine'), (5, 'bf16x3', -1, 'affine'), (0, 'bf16x3', -1, 'pre_bn'), (0, 'bf16x3', -1, 'relu_affine')]
LAUNCH_PARAMS += [(i, 'bf16x3', -1, v) for v in ('plain', 'onestage') for i in NEW]
# what the coverage check of tests/test_conv_launch_cpu.py asked for on top: the (arithmetic, tile) pairs of the plane kernels that
# only a forced tile or another shape reaches
LAUNCH_PARAMS += [(2, 'bf16x3', -1, 'pre_bn'), (NEW[2], 'bf16x3', -1, 'pre_bn'), (NEW[2], 'bf16x3', 2, 'pre_bn'), (0, 'bf16x3', 5, 'pre_bn')]
LAUNCH_PARAMS += [(NEW[2], 'bf16x3', 2, 'plain'), (NEW[2], 'bf16x2', -1, 'plain'), (NEW[3], 'bf16x1', 0, 'plain'), (NEW[3], 'bf16x1', 1, 'plain')]
LAUNCH_PARAMS += [(i, m, -1, 'plain') for i in (2, 5) for m in ('bf16x1', 'bf16x2')]
# the tile prologues and K-step state, per kernel family (forced tile 6 = none: the conv_*_x3 kernels where a plane tile would run):
# stride 2 on an odd size with a K split (conv_fprop_x3_kernel) and through the parity classes of conv_dgrad_pl_kernel; the temporal
# shift together with K-split remainder tiles in the x3, the fp32-MFMA and the plane kernels; the ragged stem, and its temporal taps
LAUNCH_PARAMS += [(3, 'bf16x3', 6, 'plain'), (3, 'bf16x3', 1, 'plain')]
LAUNCH_PARAMS += [(PRO[0], 'bf16x3', 6, 'plain'), (PRO[0], 'f32mfma', -1, 'plain'), (PRO[0], 'bf16x3', -1, 'plain')]
LAUNCH_PARAMS += [(PRO[1], 'f32mfma', -1, 'plain'), (PRO[2], 'bf16x3', -1, 'plain')]


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def _bits(shape, gen):
    return torch.from_numpy(np.packbits((torch.randn(shape, generator=gen) > 0).numpy().reshape(-1), bitorder='little').view(np.int32).copy())


@contextlib.contextmanager
def _setup(mode, tile, variant):
    """The arithmetic, the forced tile and (variant 'onestage') BDVCIL_WGRAD_2STAGE=0, which the library reads per call."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import check, lib
    saved = os.environ.get('BDVCIL_WGRAD_2STAGE')
    K.set_conv_arith(mode)
    check(lib().bdv_conv_debug_force_tile(tile), 'bdv_conv_debug_force_tile')
    if variant == 'onestage':
        os.environ['BDVCIL_WGRAD_2STAGE'] = '0'
    try:
        yield K
    finally:
        os.environ.pop('BDVCIL_WGRAD_2STAGE', None)
        if saved is not None:
            os.environ['BDVCIL_WGRAD_2STAGE'] = saved
        check(lib().bdv_conv_debug_force_tile(-1), 'bdv_conv_debug_force_tile')
        K.set_conv_arith('bf16x3')


def conv_hashes(si, mode, tile, dev, variant='plain'):
    N, H, W, Cin, Cout, R, st, pad, T, fold = ALL_SHAPES[si][:10]
    rt, st_t = ALL_SHAPES[si][10:] or (0, 0)
    gen = torch.Generator().manual_seed(4000 + si)
    x = torch.randn(N * max(st_t, 1), H, W, Cin, generator=gen)
    if Cin == 4:
        x[..., 3] = 0
    w = torch.randn(Cout, max(rt, 1) * R, R, Cin, generator=gen) / (Cin * R * R) ** 0.5
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    dy = torch.randn(N, Ho, Wo, Cout, generator=gen)
    add = torch.randn(N, H, W, Cin, generator=gen)
    yprev = torch.randn(N, H, W, Cin, generator=gen)
    mean, invstd = torch.randn(Cin, generator=gen), torch.rand(Cin, generator=gen) + 0.5
    if mode == 'bf16':                       # bf16 storage: the same values, rounded on the CPU
        x, dy, add, yprev = (t.to(torch.bfloat16) for t in (x, dy, add, yprev))
    tag = f'bits-{si}-{mode}-{tile}'       # a workspace of its own: the K-split must not depend on what ran before in the process
    out = {}
    with _setup(mode, tile, variant) as K:
        g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold, rt=rt, st_t=st_t)
        xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
        if variant in ('plain', 'onestage'):
            y, part = K.conv_fprop(xd, wd, g, bn_stats=True, ws_tag=tag)
            out['fprop'], out['fprop_stats'] = _sha(y), _sha(part)
            if Cin % 64 == 0:
                add_mask, relu_mask = _bits((N, H, W, Cin), gen).to(dev), _bits((N, H, W, Cin), gen).to(dev)
                fused = st == 1 or R >= 2            # stride 2 with a 1x1 filter takes no fused statistics
                bn = (yprev.to(dev), relu_mask, mean.to(dev), invstd.to(dev)) if fused else None
                r = K.conv_dgrad(dyd, wd, g, add_src=add.to(dev), add_mask_src=add_mask, bn_stats=bn, ws_tag=tag)
                dx, dpart = r if fused else (r, None)
                out['dgrad'] = _sha(dx)
                if fused:
                    out['dgrad_stats'] = _sha(dpart)
            out['wgrad'] = _sha(K.conv_wgrad(dyd, xd, g, ws_tag=tag))
        else:                                # operands of the fused forms, from a generator of their own
            gen2 = torch.Generator().manual_seed(5000 + si)
            if variant == 'affine':
                scale, shift = (torch.rand(Cout, generator=gen2) + 0.5).to(dev), torch.randn(Cout, generator=gen2).to(dev)
                res = torch.randn(N, Ho, Wo, Cout, generator=gen2).to(dev)
                out['fprop_affine'] = _sha(K.conv_fprop(xd, wd, g, affine=(scale, shift, res, True), ws_tag=tag))
            elif variant == 'pre_bn':
                pre = ((torch.rand(Cin, generator=gen2) + 0.5).to(dev), torch.randn(Cin, generator=gen2).to(dev))
                y, part = K.conv_fprop(xd, wd, g, bn_stats=True, pre_bn=pre, ws_tag=tag)
                out['fprop_pre'], out['fprop_pre_stats'] = _sha(y), _sha(part)
                out['wgrad_pre'] = _sha(K.conv_wgrad(dyd, xd, g, pre_bn=pre, ws_tag=tag))
            else:
                assert variant == 'relu_affine'
                relu = ((torch.rand(Cin, generator=gen2) + 0.5).to(dev), torch.randn(Cin, generator=gen2).to(dev))
                add_mask = _bits((N, H, W, Cin), gen).to(dev)
                dx, dpart = K.conv_dgrad(dyd, wd, g, add_src=add.to(dev), add_mask_src=add_mask,
                                         bn_stats=(yprev.to(dev), None, mean.to(dev), invstd.to(dev), relu), ws_tag=tag)
                out['dgrad_relu_affine'], out['dgrad_relu_affine_stats'] = _sha(dx), _sha(dpart)
        torch.cuda.synchronize()
    return out


def planned_kernels(si, mode, tile, variant):
    """Host only: the kernel names ``conv_plan`` gives for the calls of ``conv_hashes`` of this case."""
    N, H, W, Cin, Cout, R, st, pad, T, fold = ALL_SHAPES[si][:10]
    rt, st_t = ALL_SHAPES[si][10:] or (0, 0)
    pre = variant == 'pre_bn'
    kinds = {'affine': ('fprop',), 'pre_bn': ('fprop', 'wgrad'), 'relu_affine': ('dgrad',)}.get(variant, ('fprop', 'dgrad', 'wgrad'))
    with _setup(mode, tile, variant) as K:
        g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold, rt=rt, st_t=st_t)
        g.act_dtype = 1 if mode == 'bf16' else 0
        return [K.conv_plan(g, kind, pre=pre).kernel.decode() for kind in kinds if kind != 'dgrad' or Cin % 64 == 0]


def _key(si, mode, tile):
    return f'{"x".join(map(str, SHAPES[si]))}/{mode}/tile{tile}'


def _launch_key(si, mode, tile, variant):
    return f'{"x".join(map(str, ALL_SHAPES[si]))}/{mode}/tile{tile}/{variant}'


@pytest.mark.parametrize('si,mode,tile', PARAMS, ids=lambda v: str(v))
def test_conv_output_bits(si, mode, tile, dev):
    with open(GOLDEN) as f:
        want = json.load(f)[_key(si, mode, tile)]
    assert conv_hashes(si, mode, tile, dev) == want


@pytest.mark.parametrize('si,mode,tile,variant', LAUNCH_PARAMS, ids=lambda v: str(v))
def test_conv_output_bits_launch(si, mode, tile, variant, dev):
    with open(GOLDEN_LAUNCH) as f:
        want = json.load(f)[_launch_key(si, mode, tile, variant)]
    assert conv_hashes(si, mode, tile, dev, variant) == want


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    launch = len(sys.argv) > 1 and sys.argv[1] == 'launch'
    if launch:
        table = {_launch_key(*p): conv_hashes(*p[:3], torch.device('cuda:0'), p[3]) for p in LAUNCH_PARAMS}
    else:
        table = {_key(*p): conv_hashes(*p, torch.device('cuda:0')) for p in PARAMS}
    args = sys.argv[2:] if launch else sys.argv[1:]
    with open(args[0] if args else GOLDEN_LAUNCH if launch else GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + '\n}\n')
    print('wrote', len(table), 'cases')
