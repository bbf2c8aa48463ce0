"""The temporal-shift sweep of the conv kernels: the case list, the reference and the data of tests/test_conv_shift_gpu.py and
tests/test_conv_shift_cpu.py.

The shift is fused into every conv kernel (the forward and weight-gradient loaders read frame t +- 1 for the first 2 * fold input
channels and zeros at the clip ends; the dgrad epilogue scatters to t -+ 1).  The cases walk what the API admits and the other conv
tests leave out: clip lengths 1 .. 5 and 16, folds whose class boundaries fall inside a 32-deep K-step or inside a thread's 16-byte
unit, fold = Cin / 2 (no unshifted channel), frames of 1 .. 4 pixels (one row tile holds many clips), up to 43 clips.

The reference takes ``fold`` itself (``oracle.tsm_oracle.temporal_shift`` takes ``shift_div`` and cannot say fold 12, 20 or 100) and
stays in the dtype it is given, so fp64 inputs give the fp64 result."""
import functools

import torch
import torch.nn.functional as F

# (clips, T, H, W, Cin, Cout, R, stride, pad, fold); N = clips * T frames
CASES = (
    # clip length
    [(3, T, 3, 3, 64, 128, 1, 1, 0, 8) for T in (1, 2, 3, 4, 5)] + [(2, 16, 3, 3, 64, 128, 1, 1, 0, 8)]
    # fold
    + [(3, 3, 5, 7, 64, 64, 1, 1, 0, f) for f in (4, 12, 20, 28, 32)]
    + [(3, 3, 5, 7, 32, 128, 1, 1, 0, f) for f in (4, 16)]
    + [(3, 3, 5, 7, 128, 256, 1, 1, 0, f) for f in (4, 36, 60, 64)]
    + [(3, 3, 5, 7, 256, 128, 1, 1, 0, f) for f in (100, 128)]
    + [(3, 3, 5, 7, 256, 64, 1, 1, 0, 36), (3, 3, 5, 7, 64, 256, 1, 1, 0, 12)]
    # frame size and filter
    + [(43, 3, 1, 1, 64, 64, 1, 1, 0, 12),
       (43, 3, 1, 1, 128, 128, 3, 1, 1, 20),
       (5, 4, 2, 2, 128, 256, 3, 1, 1, 36),
       (3, 3, 7, 7, 64, 128, 3, 1, 1, 12),
       (3, 3, 7, 7, 64, 64, 3, 1, 1, 12),
       (3, 3, 5, 5, 128, 256, 3, 2, 1, 20),
       (3, 4, 4, 4, 64, 128, 3, 2, 1, 4),
       (2, 5, 9, 6, 256, 256, 3, 1, 1, 100),
       (3, 2, 6, 6, 128, 128, 1, 2, 0, 60)])

DIRS = ('fprop', 'dgrad', 'wgrad')
TILES = (-1, 0, 1, 2, 3, 4, 5)      # bdv_conv_debug_force_tile: the cost model, then every plane tile
# the exact regime: bf16-stored outputs hold integers up to 256, fp32 sums integers below 2^24
MAX_ACT, MAX_DW = 256, 2 ** 24


def case_id(case):
    return 'c{}xT{}-{}x{}-{}to{}-k{}s{}-f{}'.format(*case[:6], case[6], case[7], case[9])


def frames(case):
    return case[0] * case[1]


def out_hw(case):
    clips, T, H, W, Cin, Cout, R, st, pad, fold = case
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1


def shift_ref(x, T, fold):
    """x (clips * T, C, H, W) -> channels [0, fold) take frame t + 1, [fold, 2 fold) frame t - 1, zeros at the clip ends."""
    v = x.reshape(x.shape[0] // T, T, *x.shape[1:])
    out = v.clone()
    out[:, :-1, :fold] = v[:, 1:, :fold]
    out[:, -1, :fold] = 0
    out[:, 1:, fold:2 * fold] = v[:, :-1, fold:2 * fold]
    out[:, 0, fold:2 * fold] = 0
    return out.reshape(x.shape)


def ref64(case, x, w, dy):
    """(y, dx, dw) of the shifted convolution in fp64, NCHW / OIHW."""
    clips, T, H, W, Cin, Cout, R, st, pad, fold = case
    xx = x.double().clone().requires_grad_(True)
    ww = w.double().clone().requires_grad_(True)
    y = F.conv2d(shift_ref(xx, T, fold), ww, stride=st, padding=pad)
    y.backward(dy.double())
    return y.detach(), xx.grad, ww.grad


def geom(case, clips=None):
    from bdvcil_amd import kernels as K
    c, T, H, W, Cin, Cout, R, st, pad, fold = case
    return K.make_geom((c if clips is None else clips) * T, H, W, Cin, Cout, R, R, st, pad, T, fold)


def plan(case, kind, act_dtype=None, clips=None):
    """The library's plan in the current arithmetic, or None where it refuses (the message: ``refusal``)."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError
    g = geom(case, clips)
    g.act_dtype = (1 if K.ACT_DTYPE == torch.bfloat16 else 0) if act_dtype is None else act_dtype
    try:
        return K.conv_plan(g, kind)
    except HipExtensionError:
        return None


def refusal(case, kind):
    """The message of the refusal ``plan`` met."""
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError
    g = geom(case)
    g.act_dtype = 1 if K.ACT_DTYPE == torch.bfloat16 else 0
    try:
        K.conv_plan(g, kind)
    except HipExtensionError as e:
        return str(e)
    return None


def expected_refusal(case, mode, kind):
    """The refusals the sweep expects, and no other: the data and weight gradients need Cin % 64 == 0; bf16 storage applies one
    shift class to a thread's 8 channels, so it takes folds that are multiples of 8 only."""
    Cin, fold = case[4], case[9]
    return (kind != 'fprop' and Cin % 64 != 0) or (mode == 'bf16' and fold % 8 != 0)


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def pack_bits(keep):
    """bool (N, H, W, C) -> the 1-bit-per-element mask words of bdv_bn_apply (bit i % 32 of word i // 32, NHWC order)."""
    import numpy as np
    return torch.from_numpy(np.packbits(keep.numpy().reshape(-1), bitorder='little').view(np.int32).copy())


@functools.lru_cache(maxsize=None)
def exact_data(idx):
    """Integer operands of case ``idx`` (seed = idx): x, dy, add, y_prev in [-2, 2] ([-1, 1] for the last case), w in {-1, 0, 1},
    an integer shift / residual for the folded-BatchNorm epilogue and two random bit masks.  NCHW / OIHW except the NHWC masks."""
    case = CASES[idx]
    clips, T, H, W, Cin, Cout, R, st, pad, fold = case
    N, (Ho, Wo) = clips * T, out_hw(case)
    a = 1 if idx == len(CASES) - 1 else 2
    gen = torch.Generator().manual_seed(idx)
    d = dict(x=_ints((N, Cin, H, W), -a, a, gen), w=_ints((Cout, Cin, R, R), -1, 1, gen), dy=_ints((N, Cout, Ho, Wo), -a, a, gen),
             add=_ints((N, Cin, H, W), -a, a, gen), y_prev=_ints((N, Cin, H, W), -a, a, gen),
             shift=_ints((Cout,), -a, a, gen), res=_ints((N, Cout, Ho, Wo), -a, a, gen),
             add_keep=torch.rand(N, H, W, Cin, generator=gen) < 0.5, relu_keep=torch.rand(N, H, W, Cin, generator=gen) < 0.5)
    return d


@functools.lru_cache(maxsize=None)
def exact_ref(idx):
    """The fp64 results the exact regime compares with (all NCHW / OIHW): y, y_aff = relu(y + shift + res), dx, dx_add = dx + add
    where add_keep, the statistics sums s1 = sum(g), s2 = sum(g * y_prev) of g = dx_add where relu_keep, and dw."""
    case, d = CASES[idx], exact_data(idx)
    y, dx, dw = ref64(case, d['x'], d['w'], d['dy'])
    nchw = lambda m: m.permute(0, 3, 1, 2).double()     # noqa: E731
    dx_add = dx + d['add'].double() * nchw(d['add_keep'])
    g = dx_add * nchw(d['relu_keep'])
    return dict(y=y, y_aff=(y + d['shift'].double().view(1, -1, 1, 1) + d['res'].double()).clamp_min(0), dx=dx, dx_add=dx_add,
                s1=g.sum((0, 2, 3)), s2=(g * d['y_prev'].double()).sum((0, 2, 3)), dw=dw, g=g)


def exact_preconditions(idx):
    """On the reference alone: every bf16-stored output is an integer of magnitude <= 256, every fp32 sum one below 2^24."""
    r, d = exact_ref(idx), exact_data(idx)
    y = r['y']
    pre = y.abs().max().item() + d['shift'].abs().max().item() + d['res'].abs().max().item()
    assert y.abs().max().item() <= MAX_ACT and pre <= MAX_ACT, (idx, y.abs().max().item(), pre)
    assert r['dx'].abs().max().item() <= MAX_ACT and r['dx_add'].abs().max().item() <= MAX_ACT, (idx, r['dx_add'].abs().max().item())
    assert r['dw'].abs().max().item() < MAX_DW, (idx, r['dw'].abs().max().item())
    # the statistics: partial sums of integers; every partial sum is bounded by the sum of magnitudes
    assert r['g'].abs().sum((0, 2, 3)).max().item() < MAX_DW and (r['g'] * d['y_prev'].double()).abs().sum((0, 2, 3)).max().item() < MAX_DW
    return y.abs().max().item(), r['dx_add'].abs().max().item(), r['dw'].abs().max().item()


@functools.lru_cache(maxsize=None)
def rounded_data(idx):
    """randn operands with real significands (the integers above have empty mid / lo pieces): x, w / sqrt(Cin R R), dy."""
    case = CASES[idx]
    clips, T, H, W, Cin, Cout, R, st, pad, fold = case
    gen = torch.Generator().manual_seed(1000 + idx)
    x = torch.randn(clips * T, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, R, R, generator=gen) / (Cin * R * R) ** 0.5
    dy = torch.randn(clips * T, Cout, *out_hw(case), generator=gen)
    return x, w, dy
