"""Pooled-output distillation on the GPU (csrc/pod_kd.hip; KDPodSpatialFn / KDPodFlatFn; kd_type of the step and the loop) against
the torch formulas of tests/pod_oracle.py run in fp64 on the CPU -- never against a sibling kernel.

Inputs: cur = relu(randn), prev = relu(cur + 0.3 randn), seeded on the CPU; for bf16 storage rounded to bf16 first, and then exact in
the fp64 reference.  Shapes: tests/pod_oracle.py SPATIAL_CASES (one pixel; odd sizes; 17 channel groups = one past a slab; 56 x 56 =
the 16-accumulator column path; 32 slabs; one row; the 64 x 64 limit) and FLAT_CASES (one wave iteration to 8, 130 rows = 33 blocks).

Bars (pod_oracle.bar): floor + 4 x the deviation of the fp32 CPU run of the same formula from the fp64 run (from the two references
only), never looser than the project's caps (loss 1e-5 * |ref| + 1e-6, gradient 1e-4 * max|ref| + 1e-7); the bf16 gradient adds half a
bf16 ulp of the value per element.  The floors are worst-case counts of the kernels' own roundings times 2^-24:
  * a normalised profile entry carries ``spatial_depth`` roundings: 1 + ceil(W/4) + 2 (row: square, terms per thread, two shuffle
    levels) or 1 + ceil(H/4) + 3 (column: terms per thread, three adds across waves), the norm's share (its own sum of
    4 (ceil(H/4) + ceil(W/4)) terms per thread + 6 + 2 tree levels, halved by the root, plus the entries' error) and 2 for 1/x and the
    product;
  * loss floor, absolute: 2 spatial_depth (|p^| + |q^| = 2) + the frame sum (4 ceil((H+W) C / 1024) terms per thread + 8 levels,
    halved by the root, on a distance of at most 2);
  * gradient floor, relative to max |dcur|: (4 spatial_depth / min_n dist_n + frame sum + 6): u = d / dist takes the error of d and of
    dist, each divided by the distance;
  * pod_flat: ``flat_depth`` = 4 ceil(D/256) + 6 per sum; loss floor 2 flat_depth + 4; gradient (2 flat_depth + 8) on
    max |k| (|prev| + |cur| r), the two terms before they cancel.
These counts are worst cases and come out above the caps for all but the smallest shapes: the cap is the bar there.

Largest error / bar observed on an MI355X (recorded per test with record_property):
  pod_spatial fp32: loss 0.006 ((3, 4, 5, 3)), gradient 0.021 ((5, 64, 1, 9)); bf16 storage: loss 0.007, gradient 0.978 ((5, 64, 1, 9));
  pod_flat fp32: loss 0.015 ((1, 4)), gradient 0.042 ((3, 68)); bf16 storage: loss 0.020 ((5, 2048)), gradient 0.994 ((3, 68)).
  The bf16 gradients sit just under 1 because the kernels round to nearest: half an ulp is reached on some element of every
  tensor, and the fp32 part of the bar is what is left over (as for kd_mse in tests/test_loss_edges_gpu.py).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pod_oracle as PO

pytestmark = pytest.mark.gpu

STORAGE = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _fn():
    from bdvcil_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def _reference(kind, idx, bf16):
    """(cur64, prev64, loss64, grad64, loss deviation, gradient deviation of the fp32 CPU run, smallest frame distance)."""
    shape = (PO.SPATIAL_CASES if kind == 'spatial' else PO.FLAT_CASES)[idx]
    formula = PO.pod_spatial if kind == 'spatial' else PO.pod_flat
    cur, prev = PO.make_case(shape, seed=idx, bf16=bf16)
    out = []
    for dt in (torch.float64, torch.float32):
        a = cur.to(dt).detach().clone().requires_grad_(True)
        loss = formula(a, prev.to(dt))
        loss.backward()
        out.append((loss.detach().double(), a.grad.double()))
    (l64, g64), (l32, g32) = out
    dmin = PO.pod_spatial_closed(cur, prev)[3].min().item() if kind == 'spatial' else None
    return cur, prev, l64, g64, abs(l32.item() - l64.item()), (g32 - g64).abs().max().item(), dmin


def _to_dev(x64, dtype, dev, channels_last=True):
    x = x64.to(dtype).to(dev)
    if channels_last and x.dim() == 4:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x


def _grad_ratio(got, ref64, bar, bf16):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    per = bar + (PO.bf16_half_ulp(ref64) if bf16 else 0.0)
    return ((got - ref64).abs() / per).max().item()


@pytest.mark.parametrize('storage', list(STORAGE))
@pytest.mark.parametrize('idx', range(len(PO.SPATIAL_CASES)), ids=[str(s) for s in PO.SPATIAL_CASES])
def test_pod_spatial_against_fp64(idx, storage, dev, record_property):
    N, C, H, W = PO.SPATIAL_CASES[idx]
    bf16 = storage == 'bf16'
    cur64, prev64, l64, g64, dev_l, dev_g, dmin = _reference('spatial', idx, bf16)
    cur = _to_dev(cur64, STORAGE[storage], dev).requires_grad_(True)
    prev = _to_dev(prev64, STORAGE[storage], dev)
    loss = _fn().kd_pod_spatial(cur, prev)
    loss.backward()
    assert loss.shape == () and loss.dtype == torch.float32
    assert cur.grad.dtype == cur.dtype and cur.grad.stride() == cur.stride() and cur.grad.shape == cur.shape
    lbar = PO.bar(PO.spatial_loss_floor(C, H, W), dev_l, PO.loss_cap(l64))
    gbar = PO.bar(PO.spatial_grad_floor(C, H, W, dmin, g64.abs().max().item()), dev_g, PO.grad_cap(g64))
    rl = abs(loss.item() - l64.item()) / lbar
    rg = _grad_ratio(cur.grad, g64, gbar, bf16)
    print(f'pod_spatial {(N, C, H, W)} {storage}: loss {loss.item():.8f} ref {l64.item():.8f} err/bar {rl:.3f} (bar {lbar:.3e}); '
          f'grad err/bar {rg:.3f} (bar {gbar:.3e}, max|ref| {g64.abs().max().item():.3e}, min dist {dmin:.3f})')
    record_property('pod_spatial loss err/bar', rl)
    record_property('pod_spatial grad err/bar', rg)
    assert rl <= 1.0 and rg <= 1.0, (rl, rg)


@pytest.mark.parametrize('storage', list(STORAGE))
@pytest.mark.parametrize('idx', range(len(PO.FLAT_CASES)), ids=[str(s) for s in PO.FLAT_CASES])
def test_pod_flat_against_fp64(idx, storage, dev, record_property):
    N, D = PO.FLAT_CASES[idx]
    bf16 = storage == 'bf16'
    cur64, prev64, l64, g64, dev_l, dev_g, _ = _reference('flat', idx, bf16)
    cur = _to_dev(cur64, STORAGE[storage], dev).requires_grad_(True)
    prev = _to_dev(prev64, STORAGE[storage], dev)
    loss = _fn().kd_pod_flat(cur, prev)
    loss.backward()
    assert loss.shape == () and cur.grad.dtype == cur.dtype and cur.grad.shape == cur.shape
    lbar = PO.bar(PO.flat_loss_floor(D), dev_l, PO.loss_cap(l64))
    gbar = PO.bar(PO.flat_grad_floor(cur64, prev64), dev_g, PO.grad_cap(g64))
    rl = abs(loss.item() - l64.item()) / lbar
    rg = _grad_ratio(cur.grad, g64, gbar, bf16)
    print(f'pod_flat {(N, D)} {storage}: loss {loss.item():.8f} ref {l64.item():.8f} err/bar {rl:.3f} (bar {lbar:.3e}); '
          f'grad err/bar {rg:.3f} (bar {gbar:.3e})')
    record_property('pod_flat loss err/bar', rl)
    record_property('pod_flat grad err/bar', rg)
    assert rl <= 1.0 and rg <= 1.0, (rl, rg)
    # (N, D, 1, 1), the shape of the hooked avg_pool output: the same bits
    c4 = cur.detach().reshape(N, D, 1, 1).clone().requires_grad_(True)
    l4 = _fn().kd_pod_flat(c4, prev.reshape(N, D, 1, 1))
    l4.backward()
    assert torch.equal(l4, loss.detach()) and c4.grad.shape == (N, D, 1, 1) and torch.equal(c4.grad.reshape(N, D), cur.grad)


def _run(kind, cur, prev, g=None):
    fn = _fn().kd_pod_spatial if kind == 'spatial' else _fn().kd_pod_flat
    a = cur.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    b = prev.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss = fn(a, b)
    loss.backward(None if g is None else torch.tensor(g, device=cur.device))
    assert b.grad is None                                   # prev receives no gradient
    return loss.detach(), a.grad


@pytest.mark.parametrize('storage', list(STORAGE))
@pytest.mark.parametrize('kind', ['spatial', 'flat'])
def test_exact_cases(kind, storage, dev):
    from bdvcil_amd import kernels as K
    shape = (3, 68, 7, 7) if kind == 'spatial' else (5, 68)
    cur64, prev64 = PO.make_case(shape, seed=41, bf16=storage == 'bf16')
    cur, prev = _to_dev(cur64, STORAGE[storage], dev), _to_dev(prev64, STORAGE[storage], dev)
    loss, grad = _run(kind, cur, prev)
    assert torch.isfinite(loss) and loss.item() > 0 and grad.any()
    # two runs are bitwise equal, also over a workspace pre-filled with 0xFF
    K.workspace(1, dev, 'pod').fill_(0xFF)
    loss2, grad2 = _run(kind, cur, prev)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
    # an upstream gradient of 0.25 scales dcur as one extra multiply would
    loss3, grad3 = _run(kind, cur, prev, g=0.25)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad * 0.25)
    if kind == 'spatial':
        # cur identical to prev: loss 0 and dcur all zero
        l0, g0 = _run(kind, cur, cur)
        assert l0.item() == 0 and not g0.any()
        # an all-zero cur frame has exactly zero gradient; the other frames keep theirs bit for bit (frames are independent)
        z = cur.clone(memory_format=torch.preserve_format)
        z[1] = 0
        lz, gz = _run(kind, z, prev)
        assert torch.isfinite(lz) and not gz[1].any() and torch.equal(gz[0], grad[0]) and torch.equal(gz[2], grad[2])
    else:
        # an all-zero cur row: torch's own gradient is of order 1e6 there; finite is all that is asked
        z = cur.clone()
        z[1] = 0
        lz, gz = _run(kind, z, prev)
        assert torch.isfinite(lz) and torch.isfinite(gz.float()).all()


@pytest.mark.parametrize('storage', list(STORAGE))
def test_layouts(storage, dev):
    """A contiguous NCHW input and the channels-last view of the same values: bitwise equal loss, dcur in the input's strides."""
    cur64, prev64 = PO.make_case((3, 68, 5, 7), seed=43, bf16=storage == 'bf16')
    cl = [_to_dev(x, STORAGE[storage], dev) for x in (cur64, prev64)]
    nchw = [_to_dev(x, STORAGE[storage], dev, channels_last=False) for x in (cur64, prev64)]
    assert nchw[0].is_contiguous() and not cl[0].is_contiguous() and cl[0].permute(0, 2, 3, 1).is_contiguous()
    la, ga = _run('spatial', *cl)
    lb, gb = _run('spatial', *nchw)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert ga.stride() == cl[0].stride() and gb.stride() == nchw[0].stride()
    # rows picked by index_select(...).contiguous(), as kd_exemplar_only does
    idx = torch.tensor([2, 0], device=dev)
    lc, gc = _run('spatial', cl[0].index_select(0, idx).contiguous(), cl[1].index_select(0, idx).contiguous())
    ld, gd = _run('spatial', cl[0][[2, 0]], cl[1][[2, 0]])
    assert torch.equal(lc, ld) and torch.equal(gc, gd) and gc.is_contiguous()


def test_wrapper_refusals(dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError
    x = torch.zeros(2, 6, 3, 3, device=dev)
    with pytest.raises(HipExtensionError, match='C=6 is not a multiple of 4'):
        K.pod_spatial_fwd(x, x)
    big = torch.zeros(1, 4, 65, 2, device=dev)
    with pytest.raises(HipExtensionError, match='exceeds the 64 x 64 limit'):
        K.pod_spatial_fwd(big, big)
    with pytest.raises(ValueError, match='differ'):
        K.pod_spatial_fwd(torch.zeros(2, 8, 3, 3, device=dev), torch.zeros(2, 8, 3, 4, device=dev))
    with pytest.raises(ValueError, match='differ'):
        K.pod_spatial_fwd(torch.zeros(2, 8, 3, 3, device=dev), torch.zeros(2, 8, 3, 3, device=dev, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r'\(N, D\) or \(N, D, 1, 1\)'):
        K.pod_flat(torch.zeros(2, 8, 3, 3, device=dev), torch.zeros(2, 8, 3, 3, device=dev))


# ---- the training step ----------------------------------------------------------------------------------------------------------

NAMES = ['backbone.layer2', 'backbone.layer4', 'cls_head.avg_pool']
GRADS = ['backbone.conv1.conv.weight', 'backbone.layer4.1.conv2.conv.weight', 'cls_head.fc_cls.weights']


def _oracle_term(kind, c, p):
    is_map = c.dim() == 4 and c.shape[2] * c.shape[3] > 1
    if kind == 'pod':
        kind = 'pod_spatial' if is_map else 'pod_flat'
    return {'mse': F.mse_loss, 'pod_spatial': PO.pod_spatial, 'pod_flat': PO.pod_flat}[kind](c, p)


def _oracle_step(ref, ref_prev, rt, rpt, imgs, labels, kinds, weights, scale, exemplar_only, prevK):
    """oracle/tsm_oracle.py kd_training_step (cil.py:512-556) with the per-module loss chosen by ``kinds``."""
    losses = ref(imgs, labels, batch_data=None)
    ref_prev.eval()
    with torch.no_grad():
        ref_prev.forward_test(imgs)
    total = 0.0
    for name, kind, w in zip(NAMES, kinds, weights):
        c, p = rt.out[name], rpt.out[name].detach()
        if exemplar_only:
            idx = (labels.view(-1) < prevK).nonzero().reshape(-1)
            term = _oracle_term(kind, c.index_select(0, idx), p.index_select(0, idx)) if idx.nelement() else 0
        else:
            term = _oracle_term(kind, c, p)
        losses[name] = term
        total = total + scale * w * term
    losses['kd_loss'] = total
    losses['loss'] = total + losses['loss_cls']
    return losses


@pytest.mark.parametrize('kd_type,old_rows', [('pod', None), (['mse', 'pod_spatial', 'pod_flat'], None), ('pod', [0]), ('pod', [])],
                         ids=['pod', 'per_module', 'exemplar_only_row0', 'exemplar_only_none'])
def test_kd_step_pod(kd_type, old_rows, dev):
    """TSM-R18 pair, B = 2, T = 8, 64 x 64, K = 11, built as test_model_gpu.py::test_kd_step_and_hooks builds it, with that test's
    bars: per-module loss 1e-4 relative (1e-3 floor on the scale), total loss 1e-4, relative L2 of the parameter gradients <= 2e-2."""
    import bdvcil_amd as bd
    from oracle import tsm_oracle as O
    from test_model_gpu import _clips, _pair, _rel_l2
    K, prevK = 11, 5
    ref, mod, _ = _pair(18, 'LocalSimilarityClassifier', 'LSCLoss', K=K, dev=dev)
    ref_prev, mod_prev, _ = _pair(18, 'LocalSimilarityClassifier', 'LSCLoss', K=K, dev=dev, seed=5)
    imgs, labels = _clips(2, 8, 64, K)
    exemplar_only = old_rows is not None
    if exemplar_only:
        labels[:, 0] = torch.tensor([7, 9])
        for r in old_rows:
            labels[r, 0] = r + 1
    kinds = [kd_type] * 3 if isinstance(kd_type, str) else kd_type
    weights, scale = [0.5] * 3, 2.0
    rt, rpt = O.FeatureTap(ref, NAMES), O.FeatureTap(ref_prev, NAMES)
    ref.train()
    rl = _oracle_step(ref, ref_prev, rt, rpt, imgs, labels, kinds, weights, scale, exemplar_only, prevK)
    rl['loss'].backward()
    ch, ph = bd.OutputHook(mod, NAMES), bd.OutputHook(mod_prev, NAMES)
    mod.train()
    step = functools.partial(bd.base_training_step, mod, dict(imgs=imgs.to(dev), label=labels.to(dev)), current_task=1, prev_model=mod_prev,
                             current_hooks=ch, prev_hooks=ph, kd_modules_names=NAMES, kd_weight_by_module=weights,
                             adaptive_scale_factors=[1.0, scale], kd_exemplar_only=exemplar_only, previous_task_num_classes=prevK)
    ol = step(kd_type=kd_type)
    ol['loss'].backward()
    for n in NAMES:
        a, b = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (ol[n], rl[n]))
        print(f'{n}: {a:.8f} oracle {b:.8f}')
        assert abs(a - b) <= 1e-4 * max(1e-3, abs(b)), n
        assert (b == 0) == (old_rows == [])
    assert abs(ol['loss'].item() - rl['loss'].item()) <= 1e-4 * max(1.0, abs(rl['loss'].item()))
    rp, op = dict(ref.named_parameters()), dict(mod.named_parameters())
    for name in GRADS:
        assert _rel_l2(op[name].grad, rp[name].grad) <= 2e-2, name
    if kd_type == 'pod' and old_rows is None:
        with pytest.raises(ValueError, match="kd_type='pod_flat' for module 'backbone.layer2'"):
            step(kd_type='pod_flat')
        with pytest.raises(ValueError, match='kd_type has 2 entries for 3'):
            step(kd_type=['pod', 'pod'])


# ---- the loop -------------------------------------------------------------------------------------------------------------------

TASKS = [[4, 1], [5, 0]]
KD_NAMES = ['backbone.layer1', 'backbone.layer2', 'backbone.layer3', 'backbone.layer4', 'cls_head.avg_pool']


def _loop_config(tmp, **over):
    from test_task_loop_gpu import _model_cfg
    root = tmp / 'rawframes'
    root.mkdir(exist_ok=True)
    for name, n in (('train', 4), ('val', 2)):
        with open(tmp / f'{name}.txt', 'w') as f:
            for c in range(6):
                for k in range(n):
                    f.write(f'class{c}/{name}_v{c}_{k} {20 + 3 * k + c} {c}\n')
    opt = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0),
               lr=0.01, momentum=0.9, weight_decay=0.0001)
    cfg = dict(work_dir=str(tmp / 'work'), task_splits=TASKS, methods='base', starting_task=0, ending_task=1,
               num_epochs_per_task=2, videos_per_gpu=6, testing_videos_per_gpu=4, accumulate_grad_batches=1,
               use_cbf=False, cbf_train_backbone=False, cbf_num_epochs_per_task=1, budget_size=2, storing_methods='videos',
               budget_type='class', save_best=False, kd_modules_names=KD_NAMES, repr_hook='cls_head.avg_pool', kd_exemplar_only=False,
               kd_weight_by_module=[0.01] * 5, adaptive_scale_factors=[1.0, 1.4142],
               optimizer=opt, lr_scheduler=dict(type='MultiStepLR', params=dict(milestones=[2], gamma=0.1)),
               cbf_optimizer=dict(opt), cbf_lr_scheduler=dict(type='MultiStepLR', params=dict(milestones=[2], gamma=0.1)),
               data_root=str(root), train_ann_file=str(tmp / 'train.txt'), val_ann_file=str(tmp / 'val.txt'),
               cil_ann_file_template='{}_task_{}.txt', data=dict(features_extraction_epochs=1), model=_model_cfg(len(TASKS[0])))
    cfg.update(over)
    return cfg


class _LoopRuns:
    """Two tiny tasks (8 + 8 videos and 4 exemplars, 2 epochs each), once per ``kd_type``; every run starts from the same seeds."""

    def __init__(self, base):
        self.base, self.done = base, {}

    def get(self, key):
        if key not in self.done:
            import random
            import bdvcil_amd.heads
            import bdvcil_amd.task_loop as TL
            tmp = self.base / f'run_{key}'
            tmp.mkdir()
            torch.manual_seed(1234)
            random.seed(1234)
            np.random.seed(1234)
            bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0
            lines = []
            over = {} if key == 'absent' else dict(kd_type=key)
            loader = TL.SyntheticClipLoader('cuda', num_segments=8, size=64, seed=5)
            loop = TL.CILTaskLoop(_loop_config(tmp, **over), loader, device='cuda', seed=0, log=lambda *a: lines.append(' '.join(map(str, a))))
            history = loop.train()
            loop.close()
            self.done[key] = dict(kd_log=loop.kd_log, train_loss=[h['train_loss'] for h in history], lines=lines, kd_type=loop.kd_type)
        return self.done[key]


@pytest.fixture(scope='module')
def loop_runs(tmp_path_factory, dev):
    return _LoopRuns(tmp_path_factory.mktemp('pod_loops'))


def test_loop_with_pod(loop_runs):
    pod, absent = loop_runs.get('pod'), loop_runs.get('absent')
    assert pod['kd_type'] == 'pod' and absent['kd_type'] == 'mse'
    for run in (pod, absent):
        assert [(e['task'], e['epoch']) for e in run['kd_log']] == [(1, 0), (1, 1)]          # task 0 has no teacher
        for e in run['kd_log']:
            assert list(e['losses']) == KD_NAMES and all(np.isfinite(v) and v > 0 for v in e['losses'].values())
        assert len(run['train_loss']) == 2 and np.isfinite(np.asarray(run['train_loss'])).all()
    assert sum('KD losses (kd_type=pod)' in ln for ln in pod['lines']) == 2
    assert sum('KD losses (kd_type=mse)' in ln for ln in absent['lines']) == 2
    assert pod['train_loss'][0] == absent['train_loss'][0]                                   # task 0: no KD term, the same run
    for n in KD_NAMES:                                                                        # another loss: other values
        assert pod['kd_log'][0]['losses'][n] != absent['kd_log'][0]['losses'][n], n
        assert pod['kd_log'][0]['losses'][n] <= 2.0                                           # a distance of unit vectors / 1 - cos
    assert pod['train_loss'][1] != absent['train_loss'][1]


def test_loop_default_path_is_unchanged(loop_runs):
    """kd_type='mse' and the key absent: bit-identical logged losses."""
    mse, absent = loop_runs.get('mse'), loop_runs.get('absent')
    assert mse['kd_type'] == absent['kd_type'] == 'mse'
    assert mse['train_loss'] == absent['train_loss']
    assert mse['kd_log'] == absent['kd_log'] and len(mse['kd_log']) == 2
