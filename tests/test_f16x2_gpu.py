"""``set_conv_arith('f16x2')``: every operand of the plane conv kernels scaled by a per-tensor power of two and cut into TWO fp16 pieces,
three v_mfma_f32_32x32x16_f16 products per step, fp32 accumulate, the accumulators unscaled once before the epilogues -- fp32-level
results for the matrix work of 'bf16x2'.  An option, never the default.  The definition is tests/test_f16x2_cpu.py.

  1. exact cases: small integers times powers of two are exact in every piece and every sum, so fprop / dgrad / wgrad must EQUAL the
     fp64 convolution: a wrong scale, a missed unscaling or a layout slip cannot hide behind rounding;
  2. accuracy on realistic operands: at most 2 x the error the default 'bf16x3' shows on the same inputs, under the project's 2e-5
     bar, and 'bf16x2' at least 5 x worse wherever the fp16 kernel ran;
  3. the sites the mode leaves to three bf16 pieces are bit-identical to 'bf16x3'; zeros stay zeros; a training step is
     bit-reproducible;
  4. TSM-R18 / R50, a CIL step with feature KD and an I3D step under the rules the default arithmetic is held to."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import tsm_oracle as O
from oracle.tsm_oracle import temporal_shift

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout, R, stride, pad, T, fold): clips of 8 frames, the temporal shift on at the 1x1 sites
SHAPES = [
    (8, 14, 14, 64, 128, 1, 1, 0, 8, 8),
    (8, 14, 14, 128, 128, 3, 1, 1, 8, 0),
    (8, 28, 28, 128, 128, 3, 2, 1, 8, 0),
    (16, 7, 7, 256, 512, 1, 1, 0, 8, 32),       # 784 rows: a ragged last row tile
]
# which of (fprop, dgrad, wgrad) runs the two-fp16-piece kernel; the first shape's dgrad has 64 GEMM columns behind a 1x1 filter and
# its 64 -> 128 weight gradient has no plane tile: both keep the kernels of 'bf16x3'
F16_DIRS = [(True, False, False), (True, True, True), (True, True, True), (True, True, True)]
EXPONENTS = [(0, 0), (-40, -20), (40, 20), (-40, 40)]
DIRS = ('fprop', 'dgrad', 'wgrad')


@pytest.fixture
def arith():
    """select(mode) switches the conv arithmetic; the default comes back afterwards."""
    from bdvcil_amd import kernels as K
    prev = (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3)
    yield K.set_conv_arith
    K.set_conv_arith('bf16x3')
    K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3 = prev


def _ref64(case, x, w, dy):
    """(y, dx, dw) of the shifted convolution in fp64 (NCHW / OIHW tensors)."""
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    xx = x.double().clone().requires_grad_(True)
    ww = w.double().clone().requires_grad_(True)
    y = F.conv2d(temporal_shift(xx, T, Cin // fold) if fold > 0 else xx, ww, stride=st, padding=pad)
    y.backward(dy.double())
    return y.detach(), xx.grad, ww.grad


def _out_shape(case):
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    return N, Cout, (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1


def _run(case, x, w, dy, dev):
    """(y, dx, dw) of the HIP kernels in the current arithmetic, as fp64 NCHW / OIHW on the CPU."""
    from bdvcil_amd import kernels as K
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    y = K.conv_fprop(xd, wd, g)
    dx = K.conv_dgrad(dyd, wd, g)
    dw = K.conv_wgrad(dyd, xd, g)
    return tuple(t.cpu().permute(0, 3, 1, 2).double() for t in (y, dx, dw))


def _names(case):
    from bdvcil_amd import kernels as K
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    g = K.make_geom(N, H, W, Cin, Cout, R, R, st, pad, T, fold)
    return [K.conv_kernel_name(g, d) for d in DIRS], g


def _assert_f16_kernels(case, f16):
    names, _ = _names(case)
    for d, name, want in zip(DIRS, names, f16):
        assert name.endswith('F16Pieces>') == want and (not want or f'conv_{d}_pl_kernel<' in name), (d, name)


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@pytest.mark.parametrize('ea,ew', EXPONENTS)
@pytest.mark.parametrize('idx', range(len(SHAPES)))
def test_exact_cases(idx, ea, ew, dev, arith):
    """Activations and gradients: integers in [-8, 8] times 2^ea; weights: integers in [-4, 4] times 2^ew.  Every piece, product and
    sum (< 2^24) is exact, so the three results equal the fp64 convolution bit for bit."""
    case = SHAPES[idx]
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    gen = torch.Generator().manual_seed(17 * idx + ea + 3 * ew + 1000)
    x = _ints((N, Cin, H, W), -8, 8, gen) * 2.0 ** ea
    w = _ints((Cout, Cin, R, R), -4, 4, gen) * 2.0 ** ew
    dy = _ints(_out_shape(case), -8, 8, gen) * 2.0 ** ea
    arith('f16x2')
    _assert_f16_kernels(case, F16_DIRS[idx])
    for name, got, want in zip(('y', 'dx', 'dw'), _run(case, x, w, dy, dev), _ref64(case, x, w, dy)):
        assert torch.equal(got, want), (name, (got - want).abs().max().item(), want.abs().max().item())


@pytest.mark.parametrize('idx', range(len(SHAPES)))
def test_exact_with_an_outlier_in_each_operand(idx, dev, arith):
    """One entry of each operand 2^10 above the rest (8 * 2^10, weights 4 * 2^10): the scale follows the outlier, the rest stay
    fp16-normal (>= 2^1 after scaling) and everything is still exact.  The outliers sit in different channels / frames, so no product
    holds two of them and every sum stays below 2^24."""
    case = SHAPES[idx]
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    gen = torch.Generator().manual_seed(99 + idx)
    x = _ints((N, Cin, H, W), -8, 8, gen)
    w = _ints((Cout, Cin, R, R), -4, 4, gen)
    dy = _ints(_out_shape(case), -8, 8, gen)
    x[N - 1, Cin - 1, 1, 2] = 8.0 * 1024          # last frame, last input channel (never shifted: beyond 2 * fold)
    w[3, 5, R // 2, R // 2] = -4.0 * 1024         # output channel 3, input channel 5
    dy[0, Cout - 2, 2, 1] = -8.0 * 1024           # first frame, another output channel than the weight's
    arith('f16x2')
    for name, got, want in zip(('y', 'dx', 'dw'), _run(case, x, w, dy, dev), _ref64(case, x, w, dy)):
        assert want.abs().max().item() < 2.0 ** 24
        assert torch.equal(got, want), (name, (got - want).abs().max().item(), want.abs().max().item())


def test_a_shape_runs_with_split_k(dev, arith):
    """The weight gradients of these shapes are summed from several K slices (the plan's `splits`, from bdv_conv_plan_query): the
    unscaling happens before the partial products are written, so the exact cases above hold through the slice reduction."""
    from bdvcil_amd import kernels as K
    arith('f16x2')
    splits = []
    for case in SHAPES:
        names, g = _names(case)
        splits.append(K.conv_plan(g, 'wgrad').splits)
    assert splits[1] > 1 and splits[3] > 1 and K.conv_plan(_names(SHAPES[1])[1], 'wgrad').kernel.endswith(b'F16Pieces>'), splits


_ACC = {}


def _accuracy_inputs(idx):
    """randn post-ReLU activations, kaiming weights, gradients of magnitude 1e-6 with one 64 x outlier; the fp64 results, once."""
    if idx not in _ACC:
        case = SHAPES[idx]
        N, H, W, Cin, Cout, R, st, pad, T, fold = case
        gen = torch.Generator().manual_seed(4242 + idx)
        x = torch.randn(N, Cin, H, W, generator=gen).clamp_min(0)
        w = torch.randn(Cout, Cin, R, R, generator=gen) * (2.0 / (Cin * R * R)) ** 0.5
        dy = torch.randn(_out_shape(case), generator=gen) * 1e-6
        dy[1, 7, 3, 3] *= 64
        _ACC[idx] = (x, w, dy, _ref64(case, x, w, dy))
    return _ACC[idx]


@pytest.mark.parametrize('idx', range(len(SHAPES)))
def test_accuracy_against_fp64(idx, dev, arith):
    """Error = max |result - fp64 convolution| / max |fp64 convolution|.  'bf16x3' (the default, not code under test) is the control."""
    case = SHAPES[idx]
    x, w, dy, ref = _accuracy_inputs(idx)
    err = {}
    for mode in ('bf16x3', 'f16x2', 'bf16x2'):
        arith(mode)
        if mode == 'f16x2':
            _assert_f16_kernels(case, F16_DIRS[idx])
        got = _run(case, x, w, dy, dev)
        err[mode] = [(g - r).abs().max().item() / r.abs().max().item() for g, r in zip(got, ref)]
    print(f'[f16x2 accuracy] shape {idx}: (y, dx, dw) errors ' + ', '.join(f'{m} ' + '/'.join(f'{e:.2e}' for e in err[m]) for m in err))
    for k, name in enumerate(('y', 'dx', 'dw')):
        assert err['f16x2'][k] <= 2 * err['bf16x3'][k], (name, err)
        assert err['f16x2'][k] <= 2e-5, (name, err)
        if F16_DIRS[idx][k]:        # where the mode keeps the default's kernel there is nothing to tell apart
            assert err['bf16x2'][k] >= 5 * err['f16x2'][k], (name, err)


def test_fallback_sites_are_bit_identical_to_the_default(dev, arith):
    """The stem (Cin = 4 on NHWC4) and 64 GEMM columns behind a 1x1 filter keep three bf16 pieces: same kernels, same bits."""
    from bdvcil_amd import kernels as K
    gen = torch.Generator().manual_seed(5)
    stem = K.make_geom(8, 32, 32, 4, 64, 7, 7, 2, 3, 8, 0)
    narrow = K.make_geom(8, 14, 14, 256, 64, 1, 1, 1, 0, 8, 32)      # fprop: 64 columns
    widen = K.make_geom(8, 14, 14, 64, 256, 1, 1, 1, 0, 8, 8)        # dgrad: 64 columns
    xs = torch.randn(8, 32, 32, 4, generator=gen).to(dev)
    xs[..., 3] = 0
    ws = torch.randn(64, 7, 7, 4, generator=gen).to(dev)
    dys = torch.randn(8, 16, 16, 64, generator=gen).to(dev)
    xn, wn = torch.randn(8, 14, 14, 256, generator=gen).to(dev), torch.randn(64, 1, 1, 256, generator=gen).to(dev)
    dyw, ww = torch.randn(8, 14, 14, 256, generator=gen).to(dev), torch.randn(256, 1, 1, 64, generator=gen).to(dev)

    def run():
        return (K.conv_fprop(xs, ws, stem), K.conv_wgrad(dys, xs, stem), K.conv_fprop(xn, wn, narrow), K.conv_dgrad(dyw, ww, widen),
                [K.conv_kernel_name(stem, 'fprop'), K.conv_kernel_name(stem, 'wgrad'), K.conv_kernel_name(narrow, 'fprop'),
                 K.conv_kernel_name(widen, 'dgrad')])
    arith('bf16x3')
    want = run()
    arith('f16x2')
    got = run()
    assert got[4] == want[4] and not any(n.endswith('F16Pieces>') for n in got[4]), got[4]
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(a, b)


def test_all_zero_operands_give_zeros(dev, arith):
    from bdvcil_amd import kernels as K
    case = SHAPES[1]
    N, H, W, Cin, Cout, R, st, pad, T, fold = case
    gen = torch.Generator().manual_seed(8)
    w = torch.randn(Cout, Cin, R, R, generator=gen)
    dy = torch.randn(_out_shape(case), generator=gen)
    arith('f16x2')
    y, dx, dw = _run(case, torch.zeros(N, Cin, H, W), w, torch.zeros_like(dy), dev)
    assert not y.any() and not dx.any() and not dw.any()              # (NaN != 0 would count)
    _, _, dw = _run(case, torch.zeros(N, Cin, H, W), w, dy, dev)
    assert not dw.any()
    y, dx, _ = _run(case, torch.randn(N, Cin, H, W, generator=gen), torch.zeros_like(w), dy, dev)
    assert not y.any() and not dx.any()


def _r18(dev, seed=4, K_=9):
    import bdvcil_amd as bd
    torch.manual_seed(seed)
    cfg = O.r50_cfg(num_classes=K_, depth=18, head='LocalSimilarityClassifier', loss='LSCLoss', dropout_ratio=0.0)
    ref = O.build_model(copy.deepcopy(cfg))
    mod = bd.build_model(copy.deepcopy(cfg))
    mod.load_state_dict(ref.state_dict())
    return ref, mod.to(dev)


def test_training_step_is_bit_reproducible(dev, arith):
    """The amax words come from an integer atomicMax (order-independent) and nothing else on the path uses atomics: two runs of a full
    R18 training step from the same state agree in the loss and in every gradient, bit for bit."""
    _, mod = _r18(dev)
    gen = torch.Generator().manual_seed(106)
    x, y = torch.randn(2, 8, 3, 64, 64, generator=gen).to(dev), torch.randint(0, 9, (2, 1), generator=gen).to(dev)
    mod.train()
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    arith('f16x2')

    def run():
        mod.load_state_dict(state)
        mod.zero_grad(set_to_none=True)
        loss = mod(x, y)['loss_cls']
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}
    l1, g1 = run()
    l2, g2 = run()
    assert torch.isfinite(l1) and torch.equal(l1, l2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize('depth', [18, 50])
def test_eval_logits(depth, dev, arith):
    """2 clips x 8 frames x 64 x 64: logits within 1e-3 of the CPU oracle, arg-max equal."""
    import bdvcil_amd as bd
    torch.manual_seed(3)
    cfg = O.r50_cfg(num_classes=11, depth=depth, head='LocalSimilarityClassifier', loss='LSCLoss', dropout_ratio=0.0)
    ref = O.build_model(copy.deepcopy(cfg))
    mod = bd.build_model(copy.deepcopy(cfg))
    mod.load_state_dict(ref.state_dict())
    mod.to(dev)
    imgs = torch.randn(2, 8, 3, 64, 64, generator=torch.Generator().manual_seed(11))
    ref.eval(); mod.eval()
    arith('f16x2')
    with torch.no_grad():
        for mode in ('prob', 'score'):
            ref.test_cfg['average_clips'] = mod.test_cfg['average_clips'] = mode
            r = ref.forward_test(imgs)
            o = mod.forward_test(imgs.to(dev)).cpu()
            e = (o - r).abs().max().item()
            print(f'[f16x2 logits] R{depth} {mode}: max err {e:.2e}')
            assert e <= 1e-3, (mode, e)
            assert torch.equal(o.argmax(1), r.argmax(1))


@pytest.mark.parametrize('depth,head,loss', [(18, 'LocalSimilarityClassifier', 'LSCLoss'), (50, 'SimpleLinear', 'CrossEntropyLoss')])
def test_train_step_against_the_oracle(depth, head, loss, dev, arith):
    """One training step at 2 clips x 8 frames x 64 x 64 under the rule tests/test_model_gpu.py::test_train_step applies to the default
    arithmetic (loss, accuracies, every gradient against the fp64 oracle with its ReLU-flip accounting, BN statistics, one SGD step)."""
    from test_model_gpu import FLIP_FREE_SEED, test_train_step
    arith('f16x2')
    test_train_step(depth, head, loss, 64, 2, FLIP_FREE_SEED if depth == 18 else 0, dev, 'f16x2')


def test_cil_step_with_feature_kd(dev, arith):
    """The CIL training step with the feature-KD terms (a frozen previous model beside the student), as the default is held to."""
    from test_model_gpu import test_kd_step_and_hooks
    arith('f16x2')
    test_kd_step_and_hooks(dev)


def test_i3d_train_step(dev, arith):
    """I3D at the smallest shape of tests/test_i3d_gpu.py (8 frames, 64 x 64, 2 clips): the k x 1 temporal sites and the per-frame
    sites run the same plane kernels; the temporal stem keeps three bf16 pieces."""
    from test_i3d_gpu import test_i3d_train_step as step
    arith('f16x2')
    step(8, 64, 2, dev, 'f16x2')
