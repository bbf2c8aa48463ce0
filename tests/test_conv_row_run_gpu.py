"""The row-run activation path of the 256x64 plane tile (one LDS image per filter row, the three taps read from it; DESIGN.md
section 4.1.1) against the per-tap loader of the SAME kernel instantiation, switched with bdv_conv_debug_row_run in one process:
every output BIT of fprop (y and the fused BatchNorm partials) and of dgrad (dx with add_src, add_mask_src and the fused
BatchNorm-backward partials) must agree.  3x3, stride 1, padding 1, Cin = Cout = 64: the planner gives these sites the 256x64
tile.  The 256x128 tile does not take the path, so there is no 128-channel case.  One case is also held against torch-CPU conv2d
and autograd at the conv suites' bar, 2e-5 of the output scale."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, T, fold, arithmetic): what the shape can break
CASES = {
    'ragged-3x5x7': (3, 5, 7, 1, 0, 'bf16x3'),          # one ragged tile, 15 image-row ends and 2 frame ends inside it
    'phases-2x28x28': (2, 28, 28, 1, 0, 'bf16x3'),      # 7 tiles, tile starts at every phase of a row, last tile partial
    'wide-1x3x300': (1, 3, 300, 1, 0, 'bf16x3'),        # W > BM: tiles inside one image row, no separator
    'borders-2x9x1': (2, 9, 1, 1, 0, 'bf16x3'),         # every pixel is a border (W = 1 is below the bound: per-tap on both sides)
    'borders-2x1x9': (2, 1, 9, 1, 0, 'bf16x3'),         # H = 1
    'bound-below-2x9x2': (2, 9, 2, 1, 0, 'bf16x3'),     # rows_bound(256, 2) = 387 > 351 data rows: the geometry test falls back
    'bound-above-2x9x3': (2, 9, 3, 1, 0, 'bf16x3'),     # rows_bound(256, 3) = 344 <= 351: 85 separators in a full tile ...
    'bound-above-4x9x9': (4, 9, 9, 1, 0, 'bf16x3'),     # ... and a full tile of narrow rows (324 pixels: 28 separators, two tiles)
    'whole-tiles-2x181x182': (2, 181, 182, 1, 0, 'bf16x3'),   # 258 tiles: 256 whole ones (18 K-steps from tap 0) + 2 K-split
    'shift-6x5x7': (6, 5, 7, 3, 8, 'bf16x3'),           # temporal shift: the class is per channel, the same for the three taps
    'bf16x2-2x28x28': (2, 28, 28, 1, 0, 'bf16x2'),      # the NP = 2 instantiations take the path too
    'f16x2-2x28x28': (2, 28, 28, 1, 0, 'f16x2'),
}
C = 64


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _mask(shape, gen):
    import numpy as np
    return torch.from_numpy(np.packbits((torch.randn(shape, generator=gen) > 0).numpy().reshape(-1), bitorder='little').view(np.int32).copy())


def _inputs(name):
    N, H, W, T, fold, mode = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    t = dict(x=torch.randn(N, H, W, C, generator=gen), w=torch.randn(C, 3, 3, C, generator=gen) / (9 * C) ** 0.5,
             dy=torch.randn(N, H, W, C, generator=gen), add=torch.randn(N, H, W, C, generator=gen),
             yprev=torch.randn(N, H, W, C, generator=gen), mean=torch.randn(C, generator=gen), invstd=torch.rand(C, generator=gen) + 0.5,
             add_mask=_mask((N, H, W, C), gen), relu_mask=_mask((N, H, W, C), gen))
    return t


def _run(name, on, t, dev):
    """fprop with statistics and dgrad with every fused operand, the switch at `on`; a workspace tag per case, as the K-split
    depends on the workspace only."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import check, lib
    N, H, W, T, fold, mode = CASES[name]
    g = K.make_geom(N, H, W, C, C, 3, 3, 1, 1, T, fold)
    K.set_conv_arith(mode)
    check(lib().bdv_conv_debug_row_run(on), 'bdv_conv_debug_row_run')
    try:
        assert K.conv_kernel_name(g, 'fprop').startswith('conv_fprop_pl_kernel<256, 64, 4, 2, 2, ')
        assert K.conv_kernel_name(g, 'dgrad').startswith('conv_dgrad_pl_kernel<256, 64, 4, 2, 2, ')
        d = {k: v.to(dev) for k, v in t.items()}
        y, part = K.conv_fprop(d['x'], d['w'], g, bn_stats=True, ws_tag='rowrun-' + name)
        # (a shifted site scatters its gradient: no statistics of the previous unit in that epilogue's contract, as in the model)
        bn = (d['yprev'], d['relu_mask'], d['mean'], d['invstd']) if fold == 0 else None
        r = K.conv_dgrad(d['dy'], d['w'], g, add_src=d['add'], add_mask_src=d['add_mask'], bn_stats=bn, ws_tag='rowrun-' + name)
        dx, dpart = r if bn is not None else (r, None)
        torch.cuda.synchronize()
        return dict(y=y, part=part, dx=dx, dpart=dpart)
    finally:
        check(lib().bdv_conv_debug_row_run(1), 'bdv_conv_debug_row_run')
        K.set_conv_arith('bf16x3')


@pytest.mark.parametrize('name', list(CASES))
def test_row_run_bits_equal_per_tap(name, dev):
    t = _inputs(name)
    off, on = _run(name, 0, t, dev), _run(name, 1, t, dev)
    for k in off:
        if off[k] is not None:
            assert torch.equal(_bits(off[k]), _bits(on[k])), f'{name}: {k} differs between the per-tap loader and the row run'


@pytest.mark.parametrize('name', ['phases-2x28x28', 'whole-tiles-2x181x182'])
def test_case_plans_a_k_split(name, dev):
    """The planner cuts the K loop of the tiles of the last, partial round into slices [kb, ke) handed out as nk * i / split: with
    nk = 18 K-steps (two 32-channel chunks x nine taps) the 7 tiles of 2x28x28 are cut 9 ways, slices of 2 steps that start at
    taps 0, 2, 1, ... and cross a filter row.  The plan query does not carry the cut of a fprop / dgrad launch; what the library
    reports is the slab it needs for it: bdv_conv_workspace_bytes is 16 (no slab) for a launch without K-split and
    rem_tiles * split * 256 * 64 * 4 bytes with one.  conv_fprop / conv_dgrad hand the kernels a workspace of at least that size
    (kernels.workspace: max(need, 1 MiB)), so the launches of test_row_run_bits_equal_per_tap run the cut plan."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import lib
    N, H, W, T, fold, mode = CASES[name]
    g = K.make_geom(N, H, W, C, C, 3, 3, 1, 1, T, fold)
    for kind in (0, 1):
        assert lib().bdv_conv_workspace_bytes(ctypes.byref(g), kind) > 16


def test_row_run_against_torch_cpu(dev):
    """fprop and dgrad of the 7-tile case against torch-CPU conv2d and its autograd: 2e-5 of the output scale."""
    name = 'phases-2x28x28'
    t = _inputs(name)
    x = t['x'].permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, t['w'].permute(0, 3, 1, 2), stride=1, padding=1)
    y.backward(t['dy'].permute(0, 3, 1, 2))
    from bdvcil_amd import kernels as K
    g = K.make_geom(*CASES[name][:3], C, C, 3, 3, 1, 1)
    yd = K.conv_fprop(t['x'].to(dev), t['w'].to(dev), g, ws_tag='rowrun-cpu')
    dxd = K.conv_dgrad(t['dy'].to(dev), t['w'].to(dev), g, ws_tag='rowrun-cpu')
    for got, ref in ((yd.cpu(), y.detach().permute(0, 2, 3, 1)), (dxd.cpu(), x.grad.permute(0, 2, 3, 1))):
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        print(f'max err {err:.3e} of scale {scale:.3e} ({err / scale:.2e})')
        assert err <= 2e-5 * scale
