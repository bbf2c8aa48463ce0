"""The conv kernels' output BITS at small shapes, against hashes recorded before the dispatch went through one planner
(tests/golden/conv_bits.json; ``python tests/test_conv_bits_gpu.py`` on a GPU re-records them).  A convolution that is routed to
another kernel, another tile or another K-split sums in another order and changes the hash; parity with the CPU oracle is the
business of the other conv suites.  Inputs are seeded on the CPU.  Each shape is the smallest with a full and a partial row tile."""
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


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _bits(shape, gen):
    return torch.from_numpy(np.packbits((torch.randn(shape, generator=gen) > 0).numpy().reshape(-1), bitorder='little').view(np.int32).copy())


def conv_hashes(si, mode, tile, dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import check, lib
    N, H, W, Cin, Cout, R, st, pad, T, fold = SHAPES[si]
    gen = torch.Generator().manual_seed(4000 + si)
    g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold)
    x = torch.randn(N, H, W, Cin, generator=gen)
    if Cin == 4:
        x[..., 3] = 0
    w = torch.randn(Cout, R, R, Cin, generator=gen) / (Cin * R * R) ** 0.5
    dy = torch.randn(N, g.Ho, g.Wo, Cout, generator=gen)
    add = torch.randn(N, H, W, Cin, generator=gen)
    yprev = torch.randn(N, H, W, Cin, generator=gen)
    mean, invstd = torch.randn(Cin, generator=gen), torch.rand(Cin, generator=gen) + 0.5
    tag = f'bits-{si}-{mode}-{tile}'       # a workspace of its own: the K-split must not depend on what ran before in the process
    out = {}
    K.set_conv_arith(mode)
    check(lib().bdv_conv_debug_force_tile(tile), 'bdv_conv_debug_force_tile')
    try:
        xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
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
        torch.cuda.synchronize()
    finally:
        check(lib().bdv_conv_debug_force_tile(-1), 'bdv_conv_debug_force_tile')
        K.set_conv_arith('bf16x3')
    return out


def _key(si, mode, tile):
    return f'{"x".join(map(str, SHAPES[si]))}/{mode}/tile{tile}'


@pytest.mark.parametrize('si,mode,tile', PARAMS, ids=lambda v: str(v))
def test_conv_output_bits(si, mode, tile, dev):
    with open(GOLDEN) as f:
        want = json.load(f)[_key(si, mode, tile)]
    assert conv_hashes(si, mode, tile, dev) == want


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    table = {_key(*p): conv_hashes(*p, torch.device('cuda:0')) for p in PARAMS}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(table[k], sort_keys=True)) for k in sorted(table)) + '\n}\n')
    print('wrote', len(table), 'cases')
