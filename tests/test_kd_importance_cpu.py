"""CPU side of the time-channel importance distillation (csrc/tc_kd.hip, config key ``kd_importance``): the closed forms
the kernels implement against torch's fp64 autograd (tests/tc_kd_oracle.py), the map arithmetic, the C ABI of the four entry points and
their refusals (on their arguments, before any launch; no GPU), and the validation of the key by ``CILTaskLoop`` and the tool."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import tc_kd_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bdv_kd_tc_workspace_bytes', 'bdv_kd_tc_fwd', 'bdv_kd_tc_bwd', 'bdv_tc_sqgrad_accum')


@pytest.mark.parametrize('case', TO.CASES, ids=str)
def test_closed_form_equals_fp64_autograd(case):
    cur, prev, A = TO.make_case(case, seed=3)
    a = cur.clone().requires_grad_(True)
    b = prev.clone().requires_grad_(True)
    loss = TO.weighted_loss(a, b.detach(), A)
    loss.backward(torch.tensor(0.375, dtype=torch.float64))
    d = TO.weighted_grad(cur, prev, A, 0.375)
    assert b.grad is None and loss.dtype == torch.float64 and d.dtype == torch.float64
    assert (d - a.grad).abs().max().item() <= 1e-12 * max(1.0, a.grad.abs().max().item())
    # the sum written out element by element, rows n = b * T + t
    N, T, C = case[0], case[1], case[2]
    x, y = cur.reshape(N, C, -1), prev.reshape(N, C, -1)
    ref = sum((A[n % T].double()[:, None] * (x[n] - y[n]) ** 2).sum() for n in range(N)) / cur.numel()
    assert abs(loss.item() - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))


@pytest.mark.parametrize('case', TO.CASES, ids=str)
def test_all_ones_is_the_mse(case):
    cur, prev, A = TO.make_case(case, seed=4)
    ones = torch.ones_like(A)
    assert abs(TO.weighted_loss(cur, prev, ones).item() - F.mse_loss(cur, prev).item()) <= 1e-12
    a = cur.clone().requires_grad_(True)
    F.mse_loss(a, prev).backward()
    assert (TO.weighted_grad(cur, prev, ones) - a.grad).abs().max().item() <= 1e-12


def test_oracle_computes_in_the_dtype_of_its_inputs():
    cur, prev, A = TO.make_case(TO.CASES[2], dtype=torch.float32)
    assert TO.weighted_loss(cur, prev, A).dtype == torch.float32 and TO.weighted_grad(cur, prev, A).dtype == torch.float32
    assert TO.sqgrad_sum(cur, 3).dtype == torch.float32 and TO.sqgrad_sum(cur.double(), 3).dtype == torch.float64
    c16, _, A = TO.make_case(TO.CASES[2], bf16=True)
    assert torch.equal(c16.float().bfloat16().double(), c16) and A.dtype == torch.float32
    assert abs(A.double().mean().item() - 1.0) <= 1e-6


def test_sqgrad_sum_indexing():
    N, T, C, H, W = 6, 3, 4, 2, 2
    g = torch.zeros(N, C, H, W, dtype=torch.float64)
    g[1 * T + 2, 3, 1, 0] = 2.0                           # clip 1, segment 2, channel 3
    g[0 * T + 2, 3, 0, 1] = 1.0                           # clip 0, the same segment and channel
    S = TO.sqgrad_sum(g, T, scale=2.0)
    assert S.shape == (T, C) and S[2, 3].item() == 4 * 5.0 and S.sum().item() == 20.0


# ---- normalise / merge / mix ------------------------------------------------------------------------------------------------

def _maps(n, T=3, C=8):
    g = torch.Generator().manual_seed(77)
    return [torch.rand((T, C), generator=g) * (10.0 ** i) + 1e-3 for i in range(n)]


def test_update_normalise_merge_mix():
    from bdvcil_amd import update_kd_importance
    S0, S1, S2 = _maps(3)
    a0, m0, deg = update_kd_importance(S0, 7, None, 0, mix=0.25)
    assert not deg and a0.dtype == m0.dtype == torch.float32 and a0.device.type == 'cpu'
    assert abs(a0.double().mean().item() - 1) <= 1e-6 and abs(m0.double().mean().item() - 1) <= 1e-6
    assert torch.allclose(a0.double(), S0.double() / S0.double().mean(), rtol=1e-6)            # the count cancels
    assert torch.allclose(m0.double(), 0.75 * a0.double() + 0.25, rtol=1e-6)
    a1, _, _ = update_kd_importance(S1, 5, a0, 1)
    a2, m2, _ = update_kd_importance(S2, 9, a1, 2)
    want = sum(S.double() / S.double().mean() for S in (S0, S1, S2)) / 3                      # mean of the three normalised maps
    assert torch.allclose(a2.double(), want, rtol=1e-5) and abs(a2.double().mean().item() - 1) <= 1e-6
    assert torch.equal(m2, a2)                                                               # mix = 0
    # the oracle's function says the same
    o0, _ = TO.update(S0.double(), 7, None, 0)
    o1, _ = TO.update(S1.double(), 5, o0, 1)
    o2, om = TO.update(S2.double(), 9, o1, 2, mix=0.5)
    assert torch.allclose(a2.double(), o2, rtol=1e-5)
    assert torch.allclose(update_kd_importance(S2, 9, a1, 2, mix=0.5)[1].double(), om, rtol=1e-5)
    # mix = 1: uniform
    assert torch.equal(update_kd_importance(S1, 5, a0, 1, mix=1.0)[1], torch.ones(3, 8))


def test_update_degenerate_maps_give_ones():
    from bdvcil_amd import update_kd_importance
    ones = torch.ones(2, 4)
    for S in (torch.zeros(2, 4), torch.full((2, 4), float('nan')), torch.tensor([[1.0, float('inf'), 0, 0]] * 2)):
        a, m, deg = update_kd_importance(S, 4, None, 0, mix=0.3)
        assert deg and torch.equal(a, ones) and torch.allclose(m, ones)
        assert TO.normalise(S.double(), 4)[1]
    a, _, deg = update_kd_importance(torch.zeros(2, 4), 4, torch.full((2, 4), 1.0) + torch.tensor([[0.5, -0.5, 0, 0]] * 2), 1)
    assert deg and abs(a.mean().item() - 1) <= 1e-6 and a[0, 0].item() == 1.25              # merged with ones
    assert update_kd_importance(torch.ones(2, 4), 0, None, 0)[2]                              # no sample
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='mix'):
            update_kd_importance(ones, 1, None, 0, mix=bad)
    with pytest.raises(ValueError, match='task 1 needs the map of task 0'):
        update_kd_importance(ones, 1, None, 1)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------

def _lib():
    import bdvcil_amd as bd
    return bd._lib.lib()


def test_new_symbols_declared_bound_and_exported():
    import bdvcil_amd as bd
    with open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')) as f:
        header = f.read()
    lib = _lib()
    for name in NEW:
        m = re.search(r'\b' + name + r'\s*\(', header)
        assert m, name
        assert 'libs/cil/cil.py:519-541' in header[m.start() - 700:m.start()], name         # each entry cites the site it extends
        assert name in bd._lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert bd._lib.ABI_VERSION == lib.bdv_abi_version() == 33
    for fn in ('kd_time_channel', 'KDTimeChannelFn', 'estimate_kd_importance', 'update_kd_importance', 'KD_IMPORTANCE_TYPES'):
        assert hasattr(bd, fn)
    for fn in ('kd_tc_fwd', 'kd_tc_bwd', 'tc_sqgrad_accum'):
        assert hasattr(bd.kernels, fn)
    assert 'kd_importance' in bd.CILTaskLoop.__doc__ and 'kd_importance' in bd.base_training_step.__doc__


ONE = ctypes.c_void_p(16)         # aligned, never dereferenced
ODD = ctypes.c_void_p(20)
BIG = 1 << 40


def _refused(rc, name, code=-1):
    msg = _lib().bdv_last_error()
    assert rc == code and msg.startswith(name.encode() + b':'), (rc, msg)
    return msg


def _ws_bytes(N, T, C, H, W):
    """csrc/tc_kd.hip: the forward's per-block partials (at most 1024 blocks: 256-unit chunks of a frame x clips x segments) or the
    accumulator's fp64 (T, C) slabs, one per row partition (at most 2048 blocks: channel slabs x T x partitions), whichever is larger."""
    FU, C4 = H * W * C // 4, C // 4
    gx = min(-(-FU // 256), 1024)
    gy = max(1, min(1024 // gx, N // T, 65535))
    gz = max(1, min(1024 // (gx * gy), T, 65535))
    cgw = 64 if C4 >= 64 else 16
    slabs, RL, R = -(-C4 // cgw), 256 // cgw, N // T * H * W
    P = min(-(-R // RL), max(1, 2048 // (slabs * T)))
    return max(4 * gx * gy * gz, 8 * P * T * C)


WS_CASES = [(4, 2, 4, 1, 1), (6, 3, 8, 1, 1), (6, 3, 8, 5, 3), (16, 8, 68, 7, 7), (32, 8, 256, 14, 14), (256, 8, 256, 56, 56),
            (256, 8, 2048, 7, 7), (256, 8, 2048, 1, 1), (3, 1, 4, 300, 300), (2, 1, 4, 520, 520)]


def test_workspace_bytes():
    lib = _lib()
    for case in WS_CASES:
        assert lib.bdv_kd_tc_workspace_bytes(*case) == _ws_bytes(*case), case
    assert lib.bdv_kd_tc_workspace_bytes(32, 8, 256, 14, 14) == 8 * 196 * 8 * 256    # 196 row partitions of (8, 256) > 49 x 4 x 5 partials
    assert lib.bdv_kd_tc_workspace_bytes(2, 1, 4, 520, 520) == 8 * 2048 * 1 * 4       # 1024 x 1 partials < 2048 row partitions of (1, 4)
    for bad in ((0, 1, 4, 1, 1), (4, 0, 4, 1, 1), (4, 2, 0, 1, 1), (4, 2, 4, 0, 1), (4, 2, 4, 1, -1), (4, 2, 6, 1, 1), (5, 2, 4, 1, 1),
                (2, 1, 4, 1 << 15, 1 << 16)):
        assert lib.bdv_kd_tc_workspace_bytes(*bad) == 0, bad


def _common_refusals(call, name, with_ws):
    for kw in (dict(N=0), dict(T=0), dict(C=-4), dict(H=0), dict(W=-1)):
        assert b'bad argument' in _refused(call(**kw), name)
    assert b'C=6 is not a multiple of 4' in _refused(call(C=6), name)
    assert b'N=6 frames is not a multiple of T=4' in _refused(call(T=4), name)
    assert b'exceed 2^30' in _refused(call(N=3, T=3, C=4, H=1 << 15, W=1 << 16), name)
    if with_ws:
        for case in ((6, 3, 8, 5, 3), (4, 2, 4, 1, 1), (32, 8, 256, 14, 14)):
            need = _lib().bdv_kd_tc_workspace_bytes(*case)
            msg = _refused(call(*case, ws_bytes=need - 1), name, code=-2)
            assert b'workspace %d < required %d' % (need - 1, need) in msg


def test_fwd_refusals():
    lib, name = _lib(), 'bdv_kd_tc_fwd'

    def call(N=6, T=3, C=8, H=5, W=3, cur=ONE, prev=ONE, A=ONE, loss=ONE, ws=ONE, ws_bytes=BIG, dt=0):
        return lib.bdv_kd_tc_fwd(cur, prev, A, loss, N, T, C, H, W, ws, ws_bytes, dt, None)

    for kw in (dict(cur=None), dict(prev=None), dict(A=None), dict(loss=None), dict(ws=None)):
        assert b'bad argument' in _refused(call(**kw), name)
    _common_refusals(call, name, True)
    for kw in (dict(cur=ODD), dict(prev=ODD), dict(A=ODD), dict(ws=ODD)):
        assert b'alignment' in _refused(call(**kw), name)
    assert b'act_dtype 7' in _refused(call(dt=7), name)


def test_bwd_refusals():
    lib, name = _lib(), 'bdv_kd_tc_bwd'

    def call(N=6, T=3, C=8, H=5, W=3, cur=ONE, prev=ONE, A=ONE, g=ONE, d=ONE, dt=0):
        return lib.bdv_kd_tc_bwd(cur, prev, A, g, d, N, T, C, H, W, dt, None)

    for kw in (dict(cur=None), dict(prev=None), dict(A=None), dict(g=None), dict(d=None)):
        assert b'bad argument' in _refused(call(**kw), name)
    _common_refusals(call, name, False)
    for kw in (dict(cur=ODD), dict(prev=ODD), dict(A=ODD), dict(d=ODD)):
        assert b'alignment' in _refused(call(**kw), name)
    assert b'act_dtype -1' in _refused(call(dt=-1), name)


def test_accum_refusals():
    lib, name = _lib(), 'bdv_tc_sqgrad_accum'

    def call(N=6, T=3, C=8, H=5, W=3, g=ONE, S=ONE, ws=ONE, ws_bytes=BIG, scale=2.0):
        return lib.bdv_tc_sqgrad_accum(g, S, scale, N, T, C, H, W, ws, ws_bytes, None)

    for kw in (dict(g=None), dict(S=None), dict(ws=None)):
        assert b'bad argument' in _refused(call(**kw), name)
    _common_refusals(call, name, True)
    for kw in (dict(g=ODD), dict(S=ODD), dict(ws=ODD)):
        assert b'alignment' in _refused(call(**kw), name)


def test_wrappers_refuse_cpu_tensors():
    from bdvcil_amd import functional as Fn
    from bdvcil_amd import kernels as K
    x, A = torch.zeros(4, 8, 3, 3), torch.ones(2, 8)
    for fn, args in ((K.kd_tc_fwd, (x, x, A)), (K.kd_tc_bwd, (x, x, A, torch.ones(1))), (K.tc_sqgrad_accum, (A.clone(), x, 2.0)),
                     (Fn.kd_time_channel, (x, x, A))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(*args)


# ---- the config key -----------------------------------------------------------------------------------------------------------

def _loop_config(**over):
    cfg = dict(work_dir='/nonexistent/never_created', task_splits=[[0, 1], [2, 3]], methods='base',
               kd_modules_names=['backbone.layer4', 'cls_head.avg_pool'], kd_weight_by_module=[0.5, 0.5], adaptive_scale_factors=[1.0, 1.4],
               kd_importance=dict(type='time_channel'))
    cfg.update(over)
    return cfg


def _never(*a, **k):
    raise AssertionError('the clip loader must not be called')


REFUSED = [
    (dict(kd_importance='time_channel'), 'kd_importance must be a dict'),
    (dict(kd_importance=dict(type='time_channel', weight=2)), r"kd_importance: unknown keys \['weight'\]"),
    (dict(kd_importance=dict(type='channel')), "kd_importance: type='channel'"),
    (dict(kd_importance=dict(batches=0)), 'kd_importance: batches'),
    (dict(kd_importance=dict(batches=1.5)), 'kd_importance: batches'),
    (dict(kd_importance=dict(batches=True)), 'kd_importance: batches'),
    (dict(kd_importance=dict(mix=-0.1)), 'kd_importance: mix'),
    (dict(kd_importance=dict(mix=1.01)), 'kd_importance: mix'),
    (dict(kd_importance=dict(mix='half')), 'kd_importance: mix'),
    (dict(methods='icarl'), "kd_importance has no effect with methods='icarl'"),
    (dict(kd_modules_names=[]), 'kd_importance has no effect without kd_modules_names'),
    (dict(kd_exemplar_only=True), 'kd_importance cannot be combined with kd_exemplar_only=True'),
    (dict(kd_type='pod'), "kd_importance weights the 'mse' distillation only"),
    (dict(kd_type=['pod_spatial', 'pod_flat']), "kd_importance weights the 'mse' distillation only"),
    (dict(conv_arith='bf16'), "kd_importance cannot be combined with conv_arith='bf16'.*bf16x1"),
    (dict(model=dict(type='Recognizer3D')), 'kd_importance needs a 2D recognizer'),
]


@pytest.mark.parametrize('over,match', REFUSED, ids=[m[:40] for _, m in REFUSED])
def test_loop_validates_kd_importance_before_any_file_or_gpu_work(over, match):
    """Every refusal comes before the loop reads ``task_splits`` or builds a model: the config has no usable ``model`` key and a
    work_dir that cannot be created."""
    import bdvcil_amd as bd
    with pytest.raises(ValueError, match=match):
        bd.CILTaskLoop(_loop_config(**over), _never, device='cpu')
    assert not os.path.exists('/nonexistent')


def test_check_loop_kd_importance_values():
    from bdvcil_amd.task_loop import check_loop_kd_importance
    cfg = _loop_config()
    del cfg['kd_importance']
    assert check_loop_kd_importance(cfg) is None                                             # absent: off
    assert check_loop_kd_importance(_loop_config(kd_importance=None)) is None
    assert check_loop_kd_importance(_loop_config(methods='icarl', kd_importance=None)) is None
    assert check_loop_kd_importance(_loop_config()) == dict(type='time_channel', batches=None, mix=0.0)
    assert check_loop_kd_importance(_loop_config(kd_importance=dict(batches=3, mix=1))) == dict(type='time_channel', batches=3, mix=1)
    assert check_loop_kd_importance(_loop_config(kd_type=['pod', 'mse'], conv_arith='bf16x1'))['mix'] == 0.0


def test_step_refuses_importance_with_exemplar_only_and_unknown_modules():
    import bdvcil_amd as bd
    A = {'backbone.layer4': torch.ones(2, 4)}
    with pytest.raises(ValueError, match='kd_importance cannot be combined with kd_exemplar_only'):
        bd.base_training_step(None, {}, kd_modules_names=['backbone.layer4'], kd_exemplar_only=True, kd_importance=A)
    with pytest.raises(ValueError, match=r"kd_importance names \['backbone.layer4'\]"):
        bd.base_training_step(None, {}, kd_modules_names=['cls_head.avg_pool'], kd_importance=A)


def test_train_cil_flags():
    import tools.train_cil as T
    p = T.build_parser()
    args = p.parse_args(['cfg.py', '--kd-importance', '--kd-importance-mix', '0.25'])
    assert args.kd_importance is True and args.kd_importance_mix == 0.25
    none = p.parse_args(['cfg.py'])
    assert none.kd_importance is False and none.kd_importance_mix is None
    with pytest.raises(SystemExit):
        p.parse_args(['cfg.py', '--kd-importance-mix', 'half'])
    assert 'kd_importance' not in T.set_kd_importance({}, False, None)
    assert T.set_kd_importance({}, True, None)['kd_importance'] == dict(type='time_channel')
    assert T.set_kd_importance({}, True, 0.5)['kd_importance'] == dict(type='time_channel', mix=0.5)
    assert T.set_kd_importance(dict(kd_importance=dict(batches=4, mix=0.1)), False, 0.3)['kd_importance'] == dict(type='time_channel', batches=4, mix=0.3)
    with pytest.raises(SystemExit):
        T.set_kd_importance({}, False, 0.3)
