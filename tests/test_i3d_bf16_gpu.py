"""I3D-ResNet50 (BASELINE config 4) under bf16 activation storage (``conv_arith('bf16')``, BASELINE config 5's storage mode).

Bars:
  * pool2 (``MaxPool3d((2,1,1))``) on bf16 tensors equals BIT FOR BIT the fp32 kernel on the widened tensors: a maximum is one of
    its inputs and the backward a copy or a zero, so nothing is rounded; ``sel`` is the same word for word;
  * the 3-D stem under 'bf16' against 'bf16x1' (same filter, input and arithmetic, only the storage of pool1's output and of its
    gradient differs): the pooled tensor is the fp32 one rounded once, the parameter gradients are identical -- the bar
    test_bf16_storage_gpu.py::test_stem_tail_and_pools_carry_the_storage_type sets for the 2-D stem;
  * the model: a ratio against a control computed in the same test (test_bf16_storage_gpu.py::test_r50_step_at_full_resolution
    says why no constant is a fair bar for a random-init network on noise clips): bf16 storage may be at most 1.3 x as far from
    the fp32-level (``bf16x3``) parameter gradient as the ``bf16x1`` arithmetic on fp32 tensors already is; the same factor for the
    eval logits against the fp32 CPU oracle."""
import copy

import pytest
import torch

from oracle import i3d_oracle as I  # noqa: F401  (read-only; the models come from test_i3d_gpu._pair)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FACTOR = 1.3            # tests/test_bf16_storage_gpu.py's rule for TSM-R50; measured for I3D in test_i3d_step_under_bf16's docstring
STAGES = ['backbone.layer1', 'backbone.layer2', 'backbone.layer3', 'backbone.layer4']


def _rb(shape, gen, dev, scale=1.0):
    """random values exactly representable in bf16, as (bf16 tensor, the same values in fp32)"""
    t = (torch.randn(*shape, generator=gen) * scale).to(BF).to(dev)
    return t, t.float()


# ---- pool2 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(16, 6, 6, 64),      # tests/test_i3d_gpu.py::test_maxpool_t2
                                   (6, 7, 7, 32),       # 3 output frames of 1568 elements: no multiple of a 256-thread block's work
                                   (2, 1, 1, 32)])      # the smallest legal tensor: one sel word
def test_pool2_bit_exact(shape, dev):
    from bdvcil_amd import kernels as K
    gen = torch.Generator().manual_seed(shape[0] * 10 + shape[1])
    x16, x32 = _rb(shape, gen, dev)
    x16[0] = x16[1]                                                   # a tied pair: the first frame wins, sel stays 0 there
    x32 = x16.float()
    out32, sel32 = K.maxpool_t2_fwd(x32)
    out16, sel16 = K.maxpool_t2_fwd(x16)
    n = shape[0] // 2
    assert out16.dtype == BF and out32.dtype == torch.float32 and tuple(out16.shape) == (n,) + tuple(shape[1:])
    assert sel16.dtype == torch.int32 and sel16.numel() == out16.numel() // 32
    assert torch.equal(out16, out32.to(BF)) and torch.equal(sel16, sel32)
    pairs = x32.view(n, 2, *shape[1:])
    assert torch.equal(out32, torch.maximum(pairs[:, 0], pairs[:, 1]))             # the fp32 side against torch
    import numpy as np
    bits = torch.from_numpy(np.unpackbits(sel16.cpu().numpy().view(np.uint8), bitorder='little').astype(bool))
    assert torch.equal(bits, (pairs[:, 1] > pairs[:, 0]).reshape(-1).cpu())           # ties: bit 0
    assert not bits.view(n, -1)[0].any()
    d16, d32 = _rb(tuple(out16.shape), gen, dev)
    dx16, dx32 = K.maxpool_t2_bwd(d16, sel16), K.maxpool_t2_bwd(d32, sel32)
    assert dx16.dtype == BF and dx32.dtype == torch.float32 and tuple(dx16.shape) == tuple(shape)
    assert torch.equal(dx16, dx32.to(BF))
    won = (pairs[:, 1] > pairs[:, 0])
    want = torch.stack([torch.where(won, torch.zeros_like(d32), d32), torch.where(won, d32, torch.zeros_like(d32))], dim=1)
    assert torch.equal(dx32, want.view(shape))


def test_pool2_refuses_what_it_cannot_pair(dev):
    from bdvcil_amd import kernels as K
    for dt in (torch.float32, BF):
        with pytest.raises(ValueError):
            K.maxpool_t2_fwd(torch.zeros(3, 6, 6, 64, device=dev, dtype=dt))       # odd frame count
        with pytest.raises(ValueError):
            K.maxpool_t2_fwd(torch.zeros(2, 3, 3, 8, device=dev, dtype=dt))        # H*W*C % 32 != 0
    with pytest.raises(TypeError):
        K.maxpool_t2_fwd(torch.zeros(2, 6, 6, 64, device=dev, dtype=torch.float16))


# ---- the stem ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,T,S', [(2, 8, 32),       # T = 2 To: one launch over all 5 x 7 x 7 taps
                                   (1, 7, 32)])      # T != 2 To: five accumulated 2-D convolutions over gathered frames
def test_stem3d_carries_the_storage_type(B, T, S, dev):
    import bdvcil_amd as bd
    from bdvcil_amd import kernels as K
    from bdvcil_amd.resnet3d import _Stem3dFn
    gen = torch.Generator().manual_seed(T)
    x4 = torch.zeros(B * T, S, S, 4)
    x4[..., :3] = torch.randn(B * T, S, S, 3, generator=gen)
    x4 = x4.to(dev)
    w0 = (torch.randn(64, 3, 5, 7, 7, generator=gen) / (3 * 5 * 49) ** 0.5).to(dev)
    g0 = (torch.rand(64, generator=gen) + 0.5).to(dev)
    b0 = (torch.randn(64, generator=gen) * 0.1).to(dev)
    res = {}
    dp16 = None
    for mode in ('bf16x1', 'bf16'):
        with bd.conv_arith(mode):
            w, gamma, beta = (t.clone().requires_grad_(True) for t in (w0, g0, b0))
            bn = torch.nn.BatchNorm3d(64).to(dev).train()
            p = _Stem3dFn.apply(x4, w, gamma, beta, bn, True, T, True)
            if dp16 is None:
                dp16, _ = _rb(tuple(p.shape), torch.Generator().manual_seed(9), dev)
            p.backward(dp16.to(p.dtype))
            res[mode] = (p.detach(), w.grad, gamma.grad, beta.grad, bn.running_mean.clone(), bn.running_var.clone())
        assert K.ACT_DTYPE == torch.float32
    p32, p16 = res['bf16x1'][0], res['bf16'][0]
    assert tuple(p16.shape) == (B * 2, S // 4, S // 4, 64)              # To = 4 -> 2 frames per clip after pool1
    assert p32.dtype == torch.float32 and p16.dtype == BF and torch.equal(p16, p32.to(BF))
    for k, name in ((1, 'dw'), (2, 'dgamma'), (3, 'dbeta'), (4, 'running_mean'), (5, 'running_var')):
        a, b = res['bf16'][k], res['bf16x1'][k]
        assert a.dtype == torch.float32 and torch.equal(a, b), name
    assert res['bf16'][1].abs().max().item() > 0


# ---- the model -------------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _step(base, mode, imgs, labels):
    """One forward + backward of a copy of ``base`` under ``mode`` -> (losses, hooked stage outputs, {name: gradient})."""
    import bdvcil_amd as bd
    m = copy.deepcopy(base).train()
    with bd.conv_arith(mode), bd.OutputHook(m, STAGES) as hook:
        out = m(imgs, labels)
        out['loss_cls'].backward()
        torch.cuda.synchronize()
        stages = {n: hook.get_layer_output(n) for n in STAGES}
    return out, stages, {n: p.grad for n, p in m.named_parameters()}


def grad_distances(T, S, B, dev, seed):
    """d(mode) for 'bf16x1' and 'bf16': relative L2 distance of the whole parameter-gradient vector to the 'bf16x3' one, same seed,
    weights and batch; plus the runs themselves.  (Also called by the measurement that fills the docstring below.)"""
    from test_i3d_gpu import _pair                  # (tests/ is on sys.path: pytest rootdir import)
    _, base = _pair(9, dev, seed=seed)
    gen = torch.Generator().manual_seed(seed + 7)
    imgs = torch.randn(B, 1, 3, T, S, S, generator=gen).to(dev)
    labels = torch.randint(0, 9, (B, 1), generator=gen).to(dev)
    runs = {mode: _step(base, mode, imgs, labels) for mode in ('bf16x3', 'bf16x1', 'bf16')}
    names = [n for n, _ in base.named_parameters()]
    vec = {mode: torch.cat([runs[mode][2][n].reshape(-1) for n in names]) for mode in runs}
    d = {mode: _rel(vec[mode], vec['bf16x3']) for mode in ('bf16x1', 'bf16')}
    return d, runs, names


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('T,S,B', [(8, 64, 2),      # one frame per clip behind pool2: every temporal conv of layers 2-4 pads on both sides
                                   (16, 96, 2)])
def test_i3d_step_under_bf16(T, S, B, seed, dev):
    """One training step (forward + backward) of I3D-R50 in 'bf16x3', 'bf16x1' and 'bf16' on the same weights and batch.

    Structure: the hooked ``layer1..4`` outputs are bf16 under 'bf16' (fp32 in the other two), loss and every parameter gradient
    are fp32 and finite, none missing or all zero.  Numerics: d('bf16') <= 1.3 d('bf16x1'), d = relative L2 distance of the whole
    parameter-gradient vector to the 'bf16x3' result.

    The factor is tests/test_bf16_storage_gpu.py's TSM-R50 rule.  Measured for I3D on an MI355X (profiles/i3d_bf16.txt), ratio
    d('bf16') / d('bf16x1') for seeds 0, 1, 2: 0.932, 1.102, 1.096 at (T, S, B) = (8, 64, 2) and 1.052, 1.016, 1.073 at (16, 96, 2);
    the worst single conv weight 1.24 (layer1.0.conv1, seed 1).  None exceeds 1.3, so the factor stands as it is.  (Both distances
    are above 1: a random-init network on noise clips, see the module docstring; that is why the bar is a ratio.)"""
    d, runs, names = grad_distances(T, S, B, dev, seed=seed)
    for mode, (out, stages, grads) in runs.items():
        want = BF if mode == 'bf16' else torch.float32
        for n in STAGES:
            assert stages[n].dtype == want and stages[n].is_cuda, (mode, n, stages[n].dtype)
        assert out['loss_cls'].dtype == torch.float32 and bool(torch.isfinite(out['loss_cls']))
        for n in names:
            g = grads[n]
            assert g is not None, (mode, n)
            assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()), (mode, n)
            assert g.abs().max().item() > 0, (mode, n)
    t2 = T // 8                                                          # frames per clip behind pool2
    assert tuple(runs['bf16'][1]['backbone.layer1'].shape)[0] == B * 2 * t2 and tuple(runs['bf16'][1]['backbone.layer4'].shape)[0] == B * t2
    l3 = runs['bf16x3'][0]['loss_cls'].item()
    print(f'[i3d bf16] T={T} S={S} B={B} seed {seed}: loss bf16x3 {l3:.6f} bf16x1 {runs["bf16x1"][0]["loss_cls"].item():.6f} '
          f'bf16 {runs["bf16"][0]["loss_cls"].item():.6f}; d(bf16x1) {d["bf16x1"]:.4f} d(bf16) {d["bf16"]:.4f} '
          f'ratio {d["bf16"] / d["bf16x1"]:.4f}')
    assert d['bf16x1'] > 0
    assert d['bf16'] <= FACTOR * d['bf16x1'], d


def logit_distances(T, S, clips, dev, seed, classes=9, batch=2):
    """|logits(mode) - oracle| (L2 over all ``batch * classes`` logits) of the eval-mode model for 'bf16x3', 'bf16x1' and 'bf16'; the
    oracle is the fp32 CPU restatement on the same weights."""
    import bdvcil_amd as bd
    from test_i3d_gpu import _pair
    ref, mod = _pair(classes, dev, seed=seed)
    imgs = torch.randn(batch, clips, 3, T, S, S, generator=torch.Generator().manual_seed(seed + 3))
    ref.eval(); mod.eval()
    ref.test_cfg['average_clips'] = mod.test_cfg['average_clips'] = 'score'
    out = {}
    with torch.no_grad():
        r = ref(imgs, return_loss=False)
        for mode in ('bf16x3', 'bf16x1', 'bf16'):
            with bd.conv_arith(mode):
                out[mode] = mod(imgs.to(dev), return_loss=False).cpu()
    return {mode: (o - r).norm().item() for mode, o in out.items()}, out, r


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_i3d_eval_logits_under_bf16(seed, dev):
    """e('bf16') <= 1.3 e('bf16x1'), e(mode) = |logits(mode) - oracle| in L2 over the logits of 4 x 2 clips of 8 x 64 x 64 and 101
    classes (``average_clips='score'``: the raw scores), the oracle being oracle/i3d_oracle.py in fp32 on the CPU.

    Measured on an MI355X (profiles/i3d_bf16.txt), seeds 0, 1, 2: ratio 1.072, 1.119, 1.079 over these 404 logits.  The population
    is this large on purpose.  Over the 18 logits of test_i3d_gpu.py::test_i3d_eval_logits' smallest case (2 x 2 clips, 9 classes)
    the same three seeds give 1.092, 1.331, 1.128, and the one above 1.3 is carried by no tensor: for that seed every hooked stage
    output is 1.10 - 1.17 x as far from the 'bf16x3' one under 'bf16' as under 'bf16x1' (layer1 .. layer4: 1.103, 1.095, 1.140,
    1.171; the other seeds alike), and pool2's winners differ from the 'bf16x3' ones at 808 of 262144 elements against 725 (a
    changed winner moves a forward value by less than one rounding).  Eighteen numbers that share two feature vectors are too few
    to measure a ratio of error norms to 20 %; 404 are, and the factor stays 1.3 unchanged."""
    classes, batch = 101, 4
    e, out, r = logit_distances(8, 64, 2, dev, seed=seed, classes=classes, batch=batch)
    assert all(o.dtype == torch.float32 and o.shape == r.shape == (batch, classes) and bool(torch.isfinite(o).all()) for o in out.values())
    print(f'[i3d bf16] eval logits seed {seed}, |logits - oracle|: {e}; ratio {e["bf16"] / e["bf16x1"]:.4f}; oracle scale {r.norm().item():.4f}')
    assert e['bf16x3'] <= 1e-3 * (batch * classes) ** 0.5           # the default arithmetic is at the oracle (test_i3d_gpu's per-logit bar)
    assert e['bf16x1'] > 0
    assert e['bf16'] <= FACTOR * e['bf16x1'], e


def test_recognizer3d_leaves_the_process_as_it_found_it(dev):
    """A default-arithmetic step before and after steps under ``conv_arith('bf16')`` and ``conv_arith('f16x2')`` on the SAME model:
    identical logits and loss, so neither the cached weight planes nor the cached operand maxima carry a mode over."""
    import bdvcil_amd as bd
    from bdvcil_amd import kernels as K
    from test_i3d_gpu import _pair
    _, mod = _pair(9, dev, seed=1)
    gen = torch.Generator().manual_seed(4)
    imgs = torch.randn(2, 1, 3, 8, 64, 64, generator=gen).to(dev)
    labels = torch.randint(0, 9, (2, 1), generator=gen).to(dev)
    mod.train()

    def step():
        with bd.OutputHook(mod, ['cls_head']) as hook:
            out = mod(imgs, labels)
            out['loss_cls'].backward()
        mod.zero_grad(set_to_none=True)
        return hook.get_layer_output('cls_head').detach().clone(), out['loss_cls'].detach().clone()

    before = bd.get_conv_arith()
    state = (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3, K.PIECES, K.ACT_DTYPE)
    logits0, loss0 = step()
    seen = {}
    for mode in ('bf16', 'f16x2'):
        with bd.conv_arith(mode):
            assert bd.get_conv_arith() == mode
            seen[mode] = step()
        assert bd.get_conv_arith() == before and (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3, K.PIECES, K.ACT_DTYPE) == state
        logits1, loss1 = step()
        assert torch.equal(logits1, logits0) and torch.equal(loss1, loss0), mode
    assert not torch.equal(seen['bf16'][0], logits0)      # the block did run another arithmetic
    assert seen['bf16'][0].dtype == torch.float32
