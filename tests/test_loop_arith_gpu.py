"""The ``conv_arith`` key of ``CILTaskLoop``: two tasks of one epoch of the tiny TSM-R18 of tests/test_task_loop_gpu.py on synthetic
clips, in the default arithmetic, 'bf16' (bf16-stored activations: BASELINE config 5 is "5-task CIL + exemplar replay" in 16-bit
storage) and 'f16x2' (an fp32-level mode).

Bars: without the key (or with None) nothing changes, file for file; under a mode the loop leaves the same files with the same
keys, shapes and dtypes (parameters and BatchNorm buffers are fp32 in every mode), finite accuracy tables, and the process's
arithmetic as it found it, also when a batch raises; the first training loss of task 0 (same weights, same batch: the forward
alone) is within 10 % of the default loop's under 'bf16' (the bar tests/test_bf16_storage_gpu.py states for its loss curves)
and within 1e-4 relative under 'f16x2' (BASELINE.md's loss-parity gate)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from test_task_loop_gpu import _config
from test_task_loop_gpu import _loop as _seeded_loop   # (tests/ is on sys.path: pytest rootdir import)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _cfg(tmp, **over):
    over.setdefault('ending_task', 1)
    over.setdefault('num_epochs_per_task', 1)
    over.setdefault('videos_per_gpu', 4)               # 12 clips per task: three batches in task 0
    return _config(tmp, **over)


def _loop(cfg):
    """A loop whose run is a function of its config alone: the generators are seeded by test_task_loop_gpu._loop, and the dropout
    masks also depend on the per-process count of masks drawn so far (heads.HipDropout), reset here."""
    import bdvcil_amd
    bdvcil_amd.heads._DROPOUT_DRAWS[0] = 0
    return _seeded_loop(cfg)


def _state():
    from bdvcil_amd import kernels as K
    return (K.FPROP_X3, K.DGRAD_X3, K.WGRAD_X3, K.PIECES, K.ACT_DTYPE)


class _Run:
    """A finished two-task run with what it saw on the way: the loss of every training step, and per task the dtypes of the hooked
    stage outputs of the current model and of the teacher."""

    def __init__(self, tmp, **over):
        import bdvcil_amd as bd
        self.tmp = tmp
        self.cfg = _cfg(tmp, **over)
        self.work = self.cfg['work_dir']
        self.loop = loop = _loop(self.cfg)
        self.losses, self.hooked, self.modes = [], {}, set()
        inner = loop._training_step

        def step(batch):
            out = inner(batch)
            self.losses.append(float(out['loss'].detach()))
            self.modes.add(bd.get_conv_arith())
            if loop.use_kd:
                seen = self.hooked.setdefault(loop.current_task, set())
                seen.add(('current', loop.current_hooks.get_layer_output('backbone.layer2').dtype))
                if loop.current_task > 0:
                    seen.add(('prev', loop.prev_hooks.get_layer_output('backbone.layer2').dtype))
                    seen.add(('prev_pool', loop.prev_hooks.get_layer_output('cls_head.avg_pool').dtype))
            return out
        loop._training_step = step
        self.before = (bd.get_conv_arith(), _state())
        self.history = loop.train()
        self.after = (bd.get_conv_arith(), _state())
        # the re-test of every task's checkpoint, from a loop of its own as tools/train_cil.py does it
        self.tables = _seeded_loop(self.cfg).cil_testing(test_nme=True)
        self.after_test = (bd.get_conv_arith(), _state())


def _files(work):
    out = []
    for d, _, names in os.walk(work):
        out += [os.path.relpath(os.path.join(d, n), work) for n in names]
    return sorted(out)


def _same_files(work_a, work_b, exact):
    """Same file set; checkpoints with the same keys, shapes and dtypes (and values when ``exact``); text files equal when ``exact``."""
    assert _files(work_a) == _files(work_b)
    for rel in _files(work_a):
        pa, pb = os.path.join(work_a, rel), os.path.join(work_b, rel)
        if rel.endswith('.pt'):
            a, b = torch.load(pa, weights_only=True), torch.load(pb, weights_only=True)
            assert list(a) == list(b), rel
            for k in a:
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (rel, k, a[k].dtype, b[k].dtype)
                assert a[k].dtype == torch.float32 or not a[k].dtype.is_floating_point, (rel, k, a[k].dtype)     # (num_batches_tracked: int64)
                if exact:
                    assert torch.equal(a[k], b[k]), (rel, k)
        elif exact:
            with open(pa) as fa, open(pb) as fb:
                assert fa.read() == fb.read(), rel


def _numbers(table):
    return [float(v) for v in re.findall(r'(?<![\w.-])\d+\.\d+', table)]


def _finite_tables(run):
    for h in run.history:
        for k in ('cnn', 'nme'):
            assert len(h[k].values) == h['task'] + 1 and np.isfinite(h[k].values).all() and 0.0 <= h[k].avg <= 100.0
        assert np.isfinite(h['train_loss']).all()
    assert set(run.tables) == {'cnn', 'nme'}
    for t in run.tables.values():
        assert 'nan' not in t.lower() and 'inf' not in t.lower() and np.isfinite(_numbers(t)).all() and len(_numbers(t)) >= 3


@pytest.fixture(scope='module')
def default_run(tmp_path_factory):
    return _Run(tmp_path_factory.mktemp('arith_default'))


@pytest.fixture(scope='module')
def bf16_run(tmp_path_factory):
    return _Run(tmp_path_factory.mktemp('arith_bf16'), conv_arith='bf16')


def test_none_is_todays_behaviour(default_run, tmp_path):
    run = _Run(tmp_path, conv_arith=None)
    assert run.loop.conv_arith is None and default_run.loop.conv_arith is None
    assert run.modes == default_run.modes == {'bf16x3'}
    assert run.losses == default_run.losses
    _same_files(run.work, default_run.work, exact=True)
    assert run.tables == default_run.tables
    assert default_run.hooked[1] == {('current', torch.float32), ('prev', torch.float32), ('prev_pool', torch.float32)}


def _check_mode_run(run, ref, mode):
    assert run.loop.conv_arith == mode and run.modes == {mode}          # every training step ran under the mode
    assert run.before == run.after == run.after_test == ref.before and run.before[0] == 'bf16x3'
    assert len(run.history) == len(ref.history) == 2 and len(run.losses) == len(ref.losses)
    _same_files(run.work, ref.work, exact=False)
    _finite_tables(run)
    assert [len(_numbers(t)) for t in run.tables.values()] == [len(_numbers(t)) for t in ref.tables.values()]


def test_bf16_base_with_kd(bf16_run, default_run):
    """Method ``base`` with KD modules: task 1 runs the teacher, and the feature-MSE terms read bf16 hooked stage outputs."""
    _check_mode_run(bf16_run, default_run, 'bf16')
    assert bf16_run.hooked[0] == {('current', BF)}
    assert bf16_run.hooked[1] == {('current', BF), ('prev', BF), ('prev_pool', torch.float32)}
    a, b = bf16_run.losses[0], default_run.losses[0]
    print(f'[loop arith] base: first loss of task 0: bf16 {a:.6f}, default {b:.6f}')
    assert abs(a - b) <= 1e-1 * abs(b), (a, b)


def test_bf16_icarl(tmp_path_factory):
    ref = _Run(tmp_path_factory.mktemp('icarl_default'), methods='icarl')
    run = _Run(tmp_path_factory.mktemp('icarl_bf16'), methods='icarl', conv_arith='bf16')
    _check_mode_run(run, ref, 'bf16')
    a, b = run.losses[0], ref.losses[0]
    print(f'[loop arith] icarl: first loss of task 0: bf16 {a:.6f}, default {b:.6f}')
    assert abs(a - b) <= 1e-1 * abs(b), (a, b)


def test_f16x2(default_run, tmp_path):
    run = _Run(tmp_path, conv_arith='f16x2')
    _check_mode_run(run, default_run, 'f16x2')
    assert run.hooked[1] == {('current', torch.float32), ('prev', torch.float32), ('prev_pool', torch.float32)}
    a, b = run.losses[0], default_run.losses[0]
    print(f'[loop arith] base: first loss of task 0: f16x2 {a:.8f}, default {b:.8f}')
    assert abs(a - b) <= 1e-4 * abs(b), (a, b)


def test_the_arithmetic_is_restored_when_a_batch_raises(tmp_path):
    import bdvcil_amd as bd
    from bdvcil_amd import kernels as K
    loop = _loop(_cfg(tmp_path, conv_arith='bf16'))
    inner, calls, seen = loop.clip_loader, [], []

    def loader(infos, phase):
        calls.append(phase)
        seen.append(bd.get_conv_arith())
        if len(calls) == 3:
            raise RuntimeError('third batch')
        return inner(infos, phase)
    loop.clip_loader = loader
    K.WGRAD_X3 = False                               # a state no mode name describes must come back exactly
    try:
        before = _state()
        assert bd.get_conv_arith() == 'custom'
        with pytest.raises(RuntimeError, match='third batch'):
            loop.train()
        assert calls == ['train'] * 3 and seen == ['bf16'] * 3
        assert _state() == before and bd.get_conv_arith() == 'custom'
    finally:
        K.set_conv_arith('bf16x3')
    assert bd.get_conv_arith() == 'bf16x3'


def test_a_bf16_work_dir_retests_in_the_default_arithmetic(bf16_run):
    """Nothing on disk depends on the mode: the checkpoints, exemplar lists and class-mean files written under 'bf16' re-test with
    ``conv_arith=None`` (fp32 tensors, the default arithmetic) to tables of the same shape."""
    import bdvcil_amd as bd
    cfg = copy.deepcopy(bf16_run.cfg)
    cfg['conv_arith'] = None
    loop = _loop(cfg)
    assert loop.conv_arith is None and bd.get_conv_arith() == 'bf16x3'
    tables = loop.cil_testing(test_nme=True)
    assert set(tables) == set(bf16_run.tables)
    for k, t in tables.items():
        assert 'nan' not in t.lower() and np.isfinite(_numbers(t)).all()
        assert len(t.split('\n')) == len(bf16_run.tables[k].split('\n')) and len(_numbers(t)) == len(_numbers(bf16_run.tables[k]))


def test_bf16_with_frozen_stages_trains(tmp_path):
    """``frozen_stages`` alone sends no gradient through the frozen part: no eval-mode BatchNorm backward is needed."""
    cfg = _cfg(tmp_path, conv_arith='bf16')
    cfg['model']['backbone']['frozen_stages'] = 1
    loop = _loop(cfg)
    frozen = copy.deepcopy(loop.current_model.backbone.layer1.state_dict())
    first = copy.deepcopy(loop.current_model.backbone.layer2.state_dict())
    hist = loop.train()
    assert len(hist) == 2 and all(np.isfinite(h['train_loss']).all() for h in hist)
    after = loop.current_model.backbone.layer1.state_dict()
    assert all(torch.equal(after[k], v) for k, v in frozen.items())
    after2 = loop.current_model.backbone.layer2.state_dict()
    assert any(not torch.equal(after2[k], v) for k, v in first.items())


def test_bf16_with_a_frozen_backbone_in_cbf_trains(tmp_path):
    """Class-balanced fine-tuning with ``cbf_train_backbone=False`` (``freeze_backbone()``): only the head receives gradients."""
    loop = _loop(_cfg(tmp_path, conv_arith='bf16', use_cbf=True, cbf_train_backbone=False))
    hist = loop.train()
    assert len(hist) == 2 and 'cbf_loss' in hist[1] and np.isfinite(hist[1]['cbf_loss']).all()
    assert all(p.requires_grad for p in loop.current_model.backbone.parameters())       # unfrozen again
