"""Time-channel importance distillation on the GPU (csrc/tc_kd.hip; KDTimeChannelFn; ``kd_importance`` of the step and the loop;
``estimate_kd_importance``) against the torch formulas of tests/tc_kd_oracle.py run in fp64 on the CPU -- never against a sibling
kernel, except where the claim is bit-equality with it.

Inputs: cur = relu(randn), prev = relu(cur + 0.3 randn), A = rand + 0.1 renormalised to mean 1, seeded on the CPU; for bf16 storage
cur and prev are rounded to bf16 first and then exact in the fp64 reference.  Shapes (N, T, C, H, W): tc_kd_oracle.CASES -- one unit per
frame; an (N, D) tensor; odd sizes; 17 channel groups (no multiple of 64 channels); 32 frames of 12544 units, more than one grid
sweep of the forward (49 x 4 x 5 blocks: the segment stride runs and all 980 partial slots are summed) -- and (2, 1, 4, 520, 520),
whose frame has more than 1024 x 256 units and whose two clips share one block row, so the strides inside a frame and over the clips run too.

Bars
  * loss: 32 * 2^-24 relative, the bar tests/test_loss_edges_gpu.py holds kd_mse's forward to (oracle/step_tail_oracle.py KD_FWD_REL).
    Worst case here: three roundings per term, a 2-level sum of 4 terms, at most 4 terms per thread, a 6-level wave tree, 2 levels
    over the waves = 17, the finalize is fp64;
  * dcur, per element: 5 * 2^-24 * |ref| (KD_BWD_REL; five roundings and no sum: 2 / numel, the upstream scalar, the map entry, the
    difference, the product), plus half a bf16 ulp of the value under bf16 storage (pod_oracle.bf16_half_ulp);
  * S with random gradients: twice the error of torch's own fp32 expression on the same GPU tensor against fp64 (from the two
    references only).  The kernel squares and sums in fp64 and rounds S once;
  * the step: tests/test_pod_kd_gpu.py's bars (per-module loss 1e-4 relative with a 1e-3 floor on the scale, total loss 1e-4).

Largest error / bar observed on an MI355X (recorded per test with record_property): loss 0.051 ((4, 2, 4, 1, 1)); dcur 0.585 in fp32
((32, 8, 256, 14, 14)) and 1.000 under bf16 storage (the kernel rounds to nearest, so half a bf16 ulp is reached, as for kd_mse in
tests/test_loss_edges_gpu.py); S 0.500 ((2, 1, 4, 520, 520): the rounding of the stored value alone, which torch's result shares);
the estimator 0.231.
"""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import pod_oracle as PO
import tc_kd_oracle as TO
from oracle import step_tail_oracle as S

pytestmark = pytest.mark.gpu

STORAGE = {'fp32': torch.float32, 'bf16': torch.bfloat16}
WIDE = (2, 1, 4, 520, 520)
KERNEL_CASES = [(c, 'fp32') for c in TO.CASES + [WIDE]] + [(c, 'bf16') for c in TO.BF16_CASES]
UPSTREAM = 0.375


def _fn():
    from bdvcil_amd import functional as Fn
    return Fn


def _k():
    from bdvcil_amd import kernels as K
    return K


@functools.lru_cache(maxsize=None)
def _reference(case, bf16):
    """(cur64, prev64, A, loss64, dcur64 for an upstream gradient of 1): computed once per case, never modified."""
    cur, prev, A = TO.make_case(case, seed=len(case) + case[2], bf16=bf16)
    return cur, prev, A, TO.weighted_loss(cur, prev, A), TO.weighted_grad(cur, prev, A)


def _to_dev(x64, dtype, dev, channels_last=True):
    x = x64.to(dtype).to(dev)
    if channels_last and x.dim() == 4:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x


def _run(cur, prev, A, g=None):
    a = cur.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = prev.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    m = A.detach().clone().requires_grad_(True)
    loss = _fn().kd_time_channel(a, b, m)
    loss.backward(None if g is None else torch.tensor(g, device=cur.device))
    assert b.grad is None and m.grad is None                   # prev and the map receive no gradient
    assert loss.shape == () and loss.dtype == torch.float32
    assert a.grad.dtype == cur.dtype and a.grad.shape == cur.shape and a.grad.stride() == cur.stride()
    return loss.detach(), a.grad


def _grad_ratio(got, ref64, bf16):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    bar = S.KD_BWD_REL * ref64.abs() + (PO.bf16_half_ulp(ref64) if bf16 else 0.0)
    err = (got - ref64).abs()
    assert not err[bar == 0].any()                              # an exact zero stays one
    return (err / bar.clamp(min=1e-300)).max().item()


@pytest.mark.parametrize('case,storage', KERNEL_CASES, ids=[f'{c}-{s}' for c, s in KERNEL_CASES])
def test_loss_and_dcur_against_fp64(case, storage, dev, record_property):
    bf16 = storage == 'bf16'
    cur64, prev64, A, l64, g64 = _reference(case, bf16)
    cur, prev = _to_dev(cur64, STORAGE[storage], dev), _to_dev(prev64, STORAGE[storage], dev)
    Ad = A.to(dev)
    loss, grad = _run(cur, prev, Ad)
    rl = abs(loss.item() - l64.item()) / (S.KD_FWD_REL * abs(l64.item()))
    rg = _grad_ratio(grad, g64, bf16)
    loss2, grad2 = _run(cur, prev, Ad, g=UPSTREAM)
    rg2 = _grad_ratio(grad2, g64 * UPSTREAM, bf16)
    print(f'kd_time_channel {case} {storage}: loss {loss.item():.9e} ref {l64.item():.9e} err/bar {rl:.3f}; '
          f'dcur err/bar {rg:.3f} (upstream 1), {rg2:.3f} (upstream {UPSTREAM})')
    record_property('kd_time_channel loss err/bar', rl)
    record_property('kd_time_channel dcur err/bar', max(rg, rg2))
    assert torch.equal(loss2, loss)
    assert rl <= 1.0 and rg <= 1.0 and rg2 <= 1.0, (rl, rg, rg2)


@pytest.mark.parametrize('storage', list(STORAGE))
@pytest.mark.parametrize('case', [TO.CASES[1], TO.CASES[3]], ids=str)
def test_exact_properties(case, storage, dev):
    K = _k()
    bf16 = storage == 'bf16'
    N, T, C = case[0], case[1], case[2]
    cur64, prev64, A, _, _ = _reference(case, bf16)
    cur, prev, Ad = _to_dev(cur64, STORAGE[storage], dev), _to_dev(prev64, STORAGE[storage], dev), A.to(dev)
    loss, grad = _run(cur, prev, Ad, g=UPSTREAM)
    assert torch.isfinite(loss) and loss.item() > 0 and grad.any()
    # two runs are bitwise equal, also over a workspace pre-filled with 0xFF
    K.workspace(1, dev, 'tc').fill_(0xFF)
    loss2, grad2 = _run(cur, prev, Ad, g=UPSTREAM)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
    # A == 1: dcur is kd_mse_bwd's, bit for bit, for the same upstream scalar; the loss is the MSE in another summation order
    ones = torch.ones_like(Ad)
    l1, g1 = _run(cur, prev, ones, g=UPSTREAM)
    gs = torch.tensor([UPSTREAM], device=dev)
    assert torch.equal(g1, K.kd_mse_bwd(cur, prev, gs, 1.0))
    assert torch.equal(K.kd_tc_bwd(cur, prev, ones, gs), g1)
    mse = K.kd_mse_fwd(cur, prev)
    assert abs(l1.item() - mse.item()) <= 2 * S.KD_FWD_REL * abs(mse.item())
    # cur identical to prev: loss 0 and dcur all zero
    l0, g0 = _run(cur, cur, Ad, g=UPSTREAM)
    assert l0.item() == 0 and not g0.any()
    # zero entries of A: exactly zero dcur there, the other entries keep their bits
    Z = Ad.clone()
    Z[T - 1, :] = 0
    Z[0, 1::3] = 0
    lz, gz = _run(cur, prev, Z, g=UPSTREAM)
    zero = (Z == 0)[torch.arange(N, device=dev) % T]                                         # (N, C)
    zero = zero.reshape((N, C) + (1,) * (cur.dim() - 2)).expand_as(cur)
    assert zero.any() and not gz[zero].any() and torch.equal(gz[~zero], grad[~zero]) and 0 < lz.item() < loss.item()


@pytest.mark.parametrize('storage', list(STORAGE))
def test_layouts(storage, dev):
    """A contiguous NCHW input and the channels-last view of the same values: bitwise equal loss, dcur in the input's strides; and
    (N, D, 1, 1) against (N, D)."""
    case = TO.CASES[2]
    cur64, prev64, A, _, _ = _reference(case, storage == 'bf16')
    Ad = A.to(dev)
    cl = [_to_dev(x, STORAGE[storage], dev) for x in (cur64, prev64)]
    nchw = [_to_dev(x, STORAGE[storage], dev, channels_last=False) for x in (cur64, prev64)]
    assert nchw[0].is_contiguous() and not cl[0].is_contiguous() and cl[0].permute(0, 2, 3, 1).is_contiguous()
    la, ga = _run(*cl, Ad, g=UPSTREAM)
    lb, gb = _run(*nchw, Ad, g=UPSTREAM)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    lc, gc = _run(cl[0], nchw[1], Ad, g=UPSTREAM)                                           # one of each
    assert torch.equal(lc, la) and torch.equal(gc, ga)
    flat64 = _reference(TO.CASES[1], storage == 'bf16')
    c2, p2, A2 = (_to_dev(flat64[0], STORAGE[storage], dev), _to_dev(flat64[1], STORAGE[storage], dev), flat64[2].to(dev))
    l2, g2 = _run(c2, p2, A2)
    l4, g4 = _run(c2[:, :, None, None], p2[:, :, None, None], A2)
    assert torch.equal(l2, l4) and g4.shape == c2.shape + (1, 1) and torch.equal(g4.reshape(c2.shape), g2)


def test_wrapper_refusals(dev):
    K = _k()
    from bdvcil_amd._lib import HipExtensionError
    x = torch.zeros(4, 6, 3, 3, device=dev)
    with pytest.raises(HipExtensionError, match='C=6 is not a multiple of 4'):
        K.kd_tc_fwd(x, x, torch.ones(2, 6, device=dev))
    y = torch.zeros(4, 8, 3, 3, device=dev)
    with pytest.raises(ValueError, match='T dividing the frame count'):
        K.kd_tc_fwd(y, y, torch.ones(3, 8, device=dev))
    with pytest.raises(ValueError, match=r'expected \(T, C\)'):
        K.kd_tc_bwd(y, y, torch.ones(2, 4, device=dev), torch.ones(1, device=dev))
    with pytest.raises(ValueError, match='differ'):
        K.kd_tc_fwd(y, torch.zeros(4, 8, 3, 4, device=dev), torch.ones(2, 8, device=dev))
    with pytest.raises(TypeError):
        K.tc_sqgrad_accum(torch.zeros(2, 8, device=dev), y.bfloat16(), 2.0)                  # gradients are fp32


# ---- the accumulator -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', TO.CASES + [WIDE], ids=str)
def test_sqgrad_accum(case, dev, record_property):
    K = _k()
    N, T, C, H, W = case
    shape = TO.case_shape(case)
    B = N // T
    gen = torch.Generator().manual_seed(500 + C + N)
    # integers in -2..2: every square and every partial sum is an integer below 2^24, so S must be the fp64 value exactly --
    # the test of n mod T and of the slab layout
    gi = torch.randint(-2, 3, shape, generator=gen).double()
    want = TO.sqgrad_sum(gi, T, scale=float(B))
    assert want.max().item() < 2 ** 23
    for channels_last in (True, False):
        Sd = torch.zeros((T, C), device=dev)
        K.workspace(1, dev, 'tc').fill_(0xFF)
        out = K.tc_sqgrad_accum(Sd, _to_dev(gi, torch.float32, dev, channels_last), float(B))
        assert out is Sd and torch.equal(Sd.cpu().double(), want)
        K.tc_sqgrad_accum(Sd, _to_dev(gi, torch.float32, dev, channels_last), float(B))       # calling it again adds
        assert torch.equal(Sd.cpu().double(), 2 * want)
    # random gradients against twice torch's own fp32 error
    gr = torch.randn(shape, generator=gen)
    gd = _to_dev(gr, torch.float32, dev)
    want = TO.sqgrad_sum(gr.double(), T, scale=float(B))
    torch32 = ((gd * gd).reshape(B, T, C, -1).sum(dim=(0, 3)) * float(B * B)).cpu().double()
    bar = 2 * (torch32 - want).abs().max().item()
    Sd = torch.zeros((T, C), device=dev)
    K.tc_sqgrad_accum(Sd, gd, float(B))
    err = (Sd.cpu().double() - want).abs().max().item()
    S2 = torch.zeros((T, C), device=dev)
    K.tc_sqgrad_accum(S2, gd, float(B))
    print(f'tc_sqgrad_accum {case}: err {err:.3e}, torch fp32 err {bar / 2:.3e}, err/bar {err / max(bar, 1e-300):.3f}')
    record_property('tc_sqgrad_accum err/bar', err / max(bar, 1e-300))
    assert torch.equal(S2, Sd)                                                               # run to run
    assert err <= bar, (err, bar)


# ---- the training step ----------------------------------------------------------------------------------------------------------

NAMES = ['backbone.layer2', 'cls_head.avg_pool']          # one map, one pooled
GRADS = ['backbone.conv1.conv.weight', 'backbone.layer4.1.conv2.conv.weight', 'cls_head.fc_cls.weights']
T_SEG = 8


@pytest.fixture(scope='module')
def models(dev):
    """TSM-R18 pair, K = 11, built as tests/test_pod_kd_gpu.py builds it for its step test (the CPU oracle model is not run)."""
    from test_model_gpu import _pair
    _, mod, _ = _pair(18, 'LocalSimilarityClassifier', 'LSCLoss', K=11, dev=dev)
    _, mod_prev, _ = _pair(18, 'LocalSimilarityClassifier', 'LSCLoss', K=11, dev=dev, seed=5)
    return mod, mod_prev


def _step(models, dev, **kw):
    import bdvcil_amd as bd
    from test_model_gpu import _clips
    mod, mod_prev = models
    imgs, labels = _clips(2, T_SEG, 64, 11)
    ch, ph = bd.OutputHook(mod, NAMES), bd.OutputHook(mod_prev, NAMES)
    mod.train()
    mod.zero_grad(set_to_none=True)
    try:
        losses = bd.base_training_step(mod, dict(imgs=imgs.to(dev), label=labels.to(dev)), current_task=1, prev_model=mod_prev,
                                       current_hooks=ch, prev_hooks=ph, kd_modules_names=NAMES, kd_weight_by_module=[0.5, 0.5],
                                       adaptive_scale_factors=[1.0, 2.0], previous_task_num_classes=5, **kw)
        losses['loss'].backward()
        hooked = {n: (ch.get_layer_output(n).detach().double().cpu(), ph.get_layer_output(n).detach().double().cpu()) for n in NAMES}
    finally:
        ch.remove()
        ph.remove()
    grads = {n: p.grad.detach().clone() for n, p in mod.named_parameters() if n in GRADS}
    return {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in losses.items()}, hooked, grads


def test_step_with_importance(models, dev):
    from test_model_gpu import _rel_l2
    mod, _ = models
    plain, _, gp = _step(models, dev)
    C = {n: c for n, c in zip(NAMES, (128, 512))}
    ones = {n: torch.ones(T_SEG, C[n], device=dev) for n in NAMES}
    same, _, gs = _step(models, dev, kd_importance=ones)
    assert set(same) == set(plain)
    for k in plain:
        print(f'{k}: all-ones map {same[k]:.8f} no key {plain[k]:.8f}')
        assert abs(same[k] - plain[k]) <= 1e-4 * max(1e-3 if k in NAMES else 1.0, abs(plain[k])), k
    for n in GRADS:
        assert _rel_l2(gs[n], gp[n]) <= 2e-2, n
    gen = torch.Generator().manual_seed(9)
    maps = {}
    for n in NAMES:
        A = torch.rand((T_SEG, C[n]), generator=gen) + 0.1
        maps[n] = (A / A.mean()).float()
    got, hooked, _ = _step(models, dev, kd_importance={n: m.to(dev) for n, m in maps.items()})
    total = 0.0
    for n in NAMES:
        want = TO.weighted_loss(*hooked[n], maps[n]).item()
        print(f'{n}: {got[n]:.8f} oracle on the hooked tensors {want:.8f} (plain MSE {plain[n]:.8f})')
        assert abs(got[n] - want) <= 1e-4 * max(1e-3, abs(want)), n
        assert got[n] != plain[n]
        total += 2.0 * 0.5 * want
    assert abs(got['kd_loss'] - total) <= 1e-4 * max(1e-3, abs(total))
    # only one module named: the other keeps the plain MSE
    part, _, _ = _step(models, dev, kd_importance={NAMES[0]: maps[NAMES[0]].to(dev)})
    assert abs(part[NAMES[0]] - got[NAMES[0]]) <= 1e-4 * max(1e-3, abs(got[NAMES[0]]))
    assert abs(part[NAMES[1]] - plain[NAMES[1]]) <= 1e-4 * max(1e-3, abs(plain[NAMES[1]]))


# ---- the estimator --------------------------------------------------------------------------------------------------------------

def _model_flags(model):
    return ([m.training for m in model.modules()], [p.requires_grad for p in model.parameters()], copy.deepcopy(model.test_cfg),
            [len(m._forward_hooks) for m in model.modules()])


def _reference_sums(mod, batches, names, T):
    """The estimator's definition with torch ops: gradients through hooks of the test's own, squared and summed in fp64 (and, for the
    bar, in fp32 by torch on the GPU)."""
    import bdvcil_amd as bd
    mods = [bd.rgetattr(mod, n) for n in names]
    flags = [(m, m.training) for m in mod.modules()]
    grads_on = [(p, p.requires_grad) for p in mod.parameters()]
    outs = {}

    def tap(name):
        def hook(module, inputs, output):
            if not output.requires_grad:
                output = output.detach().requires_grad_()
            outs[name] = output
            return output
        return hook

    handles = [m.register_forward_hook(tap(n)) for m, n in zip(mods, names)]
    s64 = {n: 0 for n in names}
    s32 = {n: 0 for n in names}
    try:
        mod.eval()
        for p, _ in grads_on:
            p.requires_grad_(False)
        for batch in batches:
            B = batch['label'].shape[0]
            with torch.enable_grad():
                losses = mod.forward_train(batch['imgs'], batch['label'], batch_data=batch)
                grads = torch.autograd.grad(losses['loss_cls'], [outs[n] for n in names])
            for n, g in zip(names, grads):
                s64[n] = s64[n] + TO.sqgrad_sum(g.double().cpu(), T, scale=float(B))
                C = g.shape[1]
                s32[n] = s32[n] + (g * g).reshape(B, T, C, -1).sum(dim=(0, 3)) * float(B * B)
    finally:
        for h in handles:
            h.remove()
        for p, r in grads_on:
            p.requires_grad_(r)
        for m, t in flags:
            m.training = t
    return s64, {n: v.cpu().double() for n, v in s32.items()}


def test_estimate_kd_importance(models, dev, record_property):
    import bdvcil_amd as bd
    from test_model_gpu import _clips
    mod, _ = models
    batches = []
    for seed in (1, 2):
        imgs, labels = _clips(2, T_SEG, 64, 11, seed=seed)
        batches.append(dict(imgs=imgs.to(dev), label=labels.to(dev)))
    mod.train()
    mod.backbone.layer3.eval()                                  # a mixed state to restore
    list(mod.parameters())[3].requires_grad_(False)
    before = _model_flags(mod)
    state = copy.deepcopy(mod.state_dict())
    got = bd.estimate_kd_importance(mod, iter(batches), NAMES, T_SEG)
    assert _model_flags(mod) == before
    after = mod.state_dict()
    assert all(torch.equal(after[k], v) for k, v in state.items())          # no parameter and no BatchNorm buffer moved
    s64, s32 = _reference_sums(mod, batches, NAMES, T_SEG)
    assert _model_flags(mod) == before
    for n, C in zip(NAMES, (128, 512)):
        Sd, count = got[n]
        assert count == 4 and Sd.shape == (T_SEG, C) and Sd.dtype == torch.float32 and Sd.is_cuda
        assert torch.isfinite(Sd).all() and (Sd > 0).any()
        err = (Sd.cpu().double() - s64[n]).abs().max().item()
        bar = 2 * (s32[n] - s64[n]).abs().max().item()
        print(f'estimate_kd_importance {n}: err {err:.3e} torch fp32 err {bar / 2:.3e} err/bar {err / max(bar, 1e-300):.3f} '
              f'(max S {s64[n].max().item():.3e})')
        record_property(f'estimate {n} err/bar', err / max(bar, 1e-300))
        assert err <= bar, (n, err, bar)
    again = bd.estimate_kd_importance(mod, batches, NAMES, T_SEG)
    assert all(torch.equal(again[n][0], got[n][0]) for n in NAMES)           # run to run

    # an exception inside the forward: everything is as before, the taps are gone
    def boom(module, inputs):
        raise RuntimeError('boom')
    handle = mod.cls_head.register_forward_pre_hook(boom)
    try:
        with pytest.raises(RuntimeError, match='boom'):
            bd.estimate_kd_importance(mod, batches, NAMES, T_SEG)
    finally:
        handle.remove()
    assert _model_flags(mod) == before
    with pytest.raises(ValueError, match='rows for 2 clips x 4 segments'):
        bd.estimate_kd_importance(mod, batches, NAMES, 4)
    assert _model_flags(mod) == before
    mod.train()
    list(mod.parameters())[3].requires_grad_(True)


# ---- the loop -------------------------------------------------------------------------------------------------------------------

CHANNELS = {'backbone.layer1': 64, 'backbone.layer2': 128, 'backbone.layer3': 256, 'backbone.layer4': 512, 'cls_head.avg_pool': 512}


def _loop(tmp, lines=None, **over):
    import random
    import bdvcil_amd.heads
    import bdvcil_amd.task_loop as TL
    from test_pod_kd_gpu import _loop_config
    torch.manual_seed(1234)
    random.seed(1234)
    np.random.seed(1234)
    bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0
    loader = TL.SyntheticClipLoader('cuda', num_segments=8, size=64, seed=5)
    log = (lambda *a: None) if lines is None else (lambda *a: lines.append(' '.join(map(str, a))))
    return TL.CILTaskLoop(_loop_config(tmp, **over), loader, device='cuda', seed=0, log=log)


@pytest.fixture(scope='module')
def loop_run(tmp_path_factory, dev):
    """Two tiny tasks with the key (8 + 8 videos and 4 exemplars, 2 epochs each) and the same run without it."""
    base = tmp_path_factory.mktemp('kd_importance_loops')
    out = {}
    for key, over in (('with', dict(kd_importance=dict(type='time_channel', batches=2))), ('without', {})):
        tmp = base / key
        tmp.mkdir()
        lines = []
        loop = _loop(tmp, lines, **over)
        history = loop.train()
        loop.close()
        out[key] = dict(tmp=tmp, work=tmp / 'work', history=history, lines=lines, kd_log=loop.kd_log, ckpt0=loop.files.ckpt_file(0),
                        maps=None if loop.kd_importance is None else {n: m.cpu() for n, m in loop.kd_importance.items()})
    return out


def test_loop_estimates_and_uses_the_maps(loop_run):
    run = loop_run['with']
    path = run['work'] / 'kd_importance_task_0.pt'
    assert path.exists() and not (run['work'] / 'kd_importance_task_1.pt').exists()        # none after the last task
    maps = torch.load(path, map_location='cpu', weights_only=True)
    assert list(maps) == list(CHANNELS)
    for n, C in CHANNELS.items():
        m = maps[n]
        assert m.shape == (8, C) and m.dtype == torch.float32 and m.device.type == 'cpu'
        assert torch.isfinite(m).all() and abs(m.double().mean().item() - 1) <= 1e-5 and (m >= 0).all()
        assert torch.equal(run['maps'][n], m)                                                # mix = 0: the step's map is the file's
        assert m.min() < m.max()
    records = [h for h in run['history'] if h.get('kd_importance')]
    assert len(records) == 1 and len(run['history']) == 3
    rec = records[0]
    assert rec['task'] == 0 and rec['batches'] == 2 and rec['samples'] == 8 and list(rec['modules']) == list(CHANNELS)
    for n in CHANNELS:
        assert rec['modules'][n] == dict(min=float(maps[n].min()), max=float(maps[n].max()))
    assert sum('kd_importance over 8 samples' in ln for ln in run['lines']) == 1
    tasks = [h for h in run['history'] if 'train_loss' in h]
    assert [h['task'] for h in tasks] == [0, 1]
    assert all(np.isfinite(np.asarray(h['train_loss'])).all() for h in tasks)
    assert [(e['task'], e['epoch']) for e in run['kd_log']] == [(1, 0), (1, 1)]
    for e in run['kd_log']:
        assert all(np.isfinite(v) and v > 0 for v in e['losses'].values())
    # task 1 distilled with another weighting than the plain MSE
    assert run['kd_log'][0]['losses'] != loop_run['without']['kd_log'][0]['losses']


def test_loop_without_the_key_is_unchanged(loop_run):
    a, b = loop_run['with'], loop_run['without']
    assert not list(b['work'].glob('kd_importance_task_*.pt')) and b['maps'] is None
    assert [h['task'] for h in b['history']] == [0, 1] and all('kd_importance' not in h for h in b['history'])
    # the estimation touches neither parameters nor BatchNorm buffers, and task 0 has no teacher: the same checkpoint, byte for byte
    fa, fb = a['ckpt0'], b['ckpt0']
    assert fa.exists() and fb.exists() and fa.read_bytes() == fb.read_bytes()
    assert a['history'][0]['train_loss'] == b['history'][0]['train_loss']


def test_loop_resumes_from_the_file(loop_run):
    run = loop_run['with']
    over = dict(kd_importance=dict(type='time_channel', batches=2), starting_task=1)
    loop = _loop(run['tmp'], **over)
    try:
        assert loop.current_task == 1 and set(loop.kd_importance) == set(CHANNELS)
        for n in CHANNELS:
            assert loop.kd_importance[n].is_cuda and torch.equal(loop.kd_importance[n].cpu(), run['maps'][n])
    finally:
        loop.close()
    mixed = _loop(run['tmp'], kd_importance=dict(type='time_channel', mix=0.5), starting_task=1)
    try:
        for n in CHANNELS:
            assert torch.allclose(mixed.kd_importance[n].cpu(), 0.5 * run['maps'][n] + 0.5, rtol=1e-6)
    finally:
        mixed.close()
    path = run['work'] / 'kd_importance_task_0.pt'
    hidden = path.with_suffix('.hidden')
    os.replace(path, hidden)
    try:
        with pytest.raises(FileNotFoundError, match='kd_importance_task_0.pt'):
            _loop(run['tmp'], **over)
    finally:
        os.replace(hidden, path)
