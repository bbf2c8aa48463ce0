"""CPU side of the pooled-output distillation (csrc/pod_kd.hip, kd_type='pod'): the closed-form gradients the kernels implement
against torch's fp64 autograd of the plain formulas (tests/pod_oracle.py), the C ABI of the four entry points and their refusals
(on their arguments, before any launch; no GPU), and the ``kd_type`` validation of the step and of ``CILTaskLoop``."""
import ctypes
import os
import re

import pytest
import torch

import pod_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bdv_pod_workspace_bytes', 'bdv_pod_spatial_fwd', 'bdv_pod_spatial_bwd', 'bdv_pod_flat')


def _close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _spatial_inputs():
    for i, shape in enumerate(PO.SPATIAL_CASES):
        yield str(shape), PO.make_case(shape, seed=i)
    for kind in PO.SPECIAL:
        yield kind, PO.special_case(kind)


@pytest.mark.parametrize('name,pair', list(_spatial_inputs()), ids=[n for n, _ in _spatial_inputs()])
def test_spatial_closed_form_equals_fp64_autograd(name, pair):
    cur, prev = pair
    a = cur.clone().requires_grad_(True)
    b = prev.clone().requires_grad_(True)
    loss = PO.pod_spatial(a, b.detach())
    loss.backward()
    closs, G, dcur, dist = PO.pod_spatial_closed(cur, prev)
    assert torch.isfinite(a.grad).all() and torch.isfinite(dcur).all() and b.grad is None
    assert abs(closs.item() - loss.item()) <= 1e-12
    assert _close(dcur, a.grad)
    if name == 'cur_eq_prev':
        assert loss.item() == 0 and not a.grad.any() and not dcur.any()
    if name == 'zero_cur_frame':
        assert not a.grad[1].any() and not dcur[1].any()             # dcur = 2 cur (...), whatever G is
        assert a.grad[0].any()
    if name == 'zero_prev_frame':
        assert abs(dist[1].item() - 1.0) <= 1e-12                    # | p^ - 0 | = 1


@pytest.mark.parametrize('shape', PO.FLAT_CASES + [(3, 8, 1, 1)], ids=str)
def test_flat_closed_form_equals_fp64_autograd(shape):
    cur, prev = PO.make_case(shape, seed=len(shape) + shape[1])
    a = cur.clone().requires_grad_(True)
    loss = PO.pod_flat(a, prev)
    loss.backward()
    closs, dcur = PO.pod_flat_closed(cur, prev)
    assert abs(closs.item() - loss.item()) <= 1e-12 and _close(dcur, a.grad)
    same_loss, same_d = PO.pod_flat_closed(cur, cur.clone())
    assert abs(same_loss.item()) <= 1e-12 and same_d.abs().max().item() <= 1e-12
    zc = cur.clone()
    zc[0] = 0                                                        # an all-zero row: a gradient of order 1e6 in torch itself
    z = zc.clone().requires_grad_(True)
    PO.pod_flat(z, prev).backward()
    assert torch.isfinite(z.grad).all() and torch.isfinite(PO.pod_flat_closed(zc, prev)[1]).all()


def test_oracle_computes_in_the_dtype_of_its_inputs():
    cur, prev = PO.make_case((2, 8, 3, 5), dtype=torch.float32)
    assert PO.pod_spatial(cur, prev).dtype == torch.float32 and PO.pod_flat(cur[:, :, :1, :1], prev[:, :, :1, :1]).dtype == torch.float32
    assert PO.pod_spatial(cur.double(), prev.double()).dtype == torch.float64
    c16, _ = PO.make_case((2, 8, 3, 5), bf16=True)
    assert torch.equal(c16.float().bfloat16().double(), c16)         # bf16-rounded inputs are exact in fp64
    assert PO.bf16_half_ulp(torch.tensor([1.0, 1.5, 0.0, -3.0], dtype=torch.float64)).tolist() == [2.0 ** -8, 2.0 ** -8, 0.0, 2.0 ** -7]


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
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in bd._lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert 'libs/cil/cil.py:519-541' in header[header.index('bdv_pod_workspace_bytes') - 1200:]
    assert bd._lib.ABI_VERSION == lib.bdv_abi_version()
    for fn in ('kd_pod_spatial', 'kd_pod_flat', 'KDPodSpatialFn', 'KDPodFlatFn', 'KD_TYPES'):
        assert hasattr(bd, fn)
    for fn in ('pod_spatial_fwd', 'pod_spatial_bwd', 'pod_flat'):
        assert hasattr(bd.kernels, fn)


ONE = ctypes.c_void_p(16)         # aligned, never dereferenced
ODD = ctypes.c_void_p(20)
BIG = 1 << 40


def _refused(rc, name, code=-1):
    msg = _lib().bdv_last_error()
    assert rc == code and msg.startswith(name.encode() + b':'), (rc, msg)
    return msg


def test_workspace_bytes():
    lib = _lib()
    for N, C, H, W in PO.SPATIAL_CASES + [(256, 256, 56, 56)]:
        slabs = (C // 4 + 15) // 16
        assert lib.bdv_pod_workspace_bytes(N, C, H, W) == 4 * (2 * N * (H + W) * C + 2 * N * slabs + N)
    for bad in ((0, 4, 1, 1), (1, 0, 1, 1), (1, 4, 0, 1), (1, 4, 1, -1)):
        assert lib.bdv_pod_workspace_bytes(*bad) == 0


def test_spatial_fwd_refusals():
    lib, name = _lib(), 'bdv_pod_spatial_fwd'

    def call(N=2, C=8, H=5, W=3, cur=ONE, prev=ONE, loss=ONE, G=ONE, ws=ONE, ws_bytes=BIG, dt=0):
        return lib.bdv_pod_spatial_fwd(cur, prev, loss, G, N, C, H, W, ws, ws_bytes, dt, None)

    for kw in (dict(cur=None), dict(prev=None), dict(loss=None), dict(G=None), dict(ws=None), dict(N=0), dict(C=0), dict(H=-1), dict(W=0)):
        assert b'bad argument' in _refused(call(**kw), name)
    assert b'C=6 is not a multiple of 4' in _refused(call(C=6), name)
    assert b'H=65 W=3 exceeds the 64 x 64 limit' in _refused(call(H=PO.MAX_HW + 1), name)
    assert b'H=5 W=65 exceeds the 64 x 64 limit' in _refused(call(W=PO.MAX_HW + 1), name)
    assert b'N=65536' in _refused(call(N=65536), name)
    assert b'alignment' in _refused(call(cur=ODD), name)
    assert b'act_dtype 7' in _refused(call(dt=7), name)
    for N, C, H, W in ((2, 8, 5, 3), (1, 4, 1, 1), (3, 68, 64, 64)):
        need = lib.bdv_pod_workspace_bytes(N, C, H, W)
        msg = _refused(call(N, C, H, W, ws_bytes=need - 1), name, code=-2)
        assert b'workspace %d < required %d' % (need - 1, need) in msg


def test_spatial_bwd_refusals():
    lib, name = _lib(), 'bdv_pod_spatial_bwd'

    def call(N=2, C=8, H=5, W=3, cur=ONE, G=ONE, g=ONE, d=ONE, dt=0):
        return lib.bdv_pod_spatial_bwd(cur, G, g, d, N, C, H, W, dt, None)

    for kw in (dict(cur=None), dict(G=None), dict(g=None), dict(d=None), dict(N=0), dict(C=-4), dict(H=0), dict(W=0)):
        assert b'bad argument' in _refused(call(**kw), name)
    assert b'C=10 is not a multiple of 4' in _refused(call(C=10), name)
    assert b'exceeds the 64 x 64 limit' in _refused(call(H=65), name)
    assert b'exceeds the 64 x 64 limit' in _refused(call(W=100), name)
    assert b'alignment' in _refused(call(d=ODD), name)
    assert b'act_dtype -1' in _refused(call(dt=-1), name)


def test_flat_refusals():
    lib, name = _lib(), 'bdv_pod_flat'

    def call(N=3, D=8, cur=ONE, prev=ONE, loss=ONE, d=ONE, ws=ONE, ws_bytes=BIG, dt=0):
        return lib.bdv_pod_flat(cur, prev, loss, d, N, D, ws, ws_bytes, dt, None)

    for kw in (dict(cur=None), dict(prev=None), dict(loss=None), dict(d=None), dict(ws=None), dict(N=0), dict(D=0)):
        assert b'bad argument' in _refused(call(**kw), name)
    assert b'D=66 is not a multiple of 4' in _refused(call(D=66), name)
    assert b'alignment' in _refused(call(prev=ODD), name)
    assert b'act_dtype 2' in _refused(call(dt=2), name)
    need = lib.bdv_pod_workspace_bytes(3, 8, 1, 1)
    assert b'workspace %d < required %d' % (need - 1, need) in _refused(call(ws_bytes=need - 1), name, code=-2)


def test_wrappers_refuse_cpu_tensors():
    from bdvcil_amd import kernels as K
    x = torch.zeros(2, 4, 3, 3)
    for fn, args in ((K.pod_spatial_fwd, (x, x)), (K.pod_spatial_bwd, (x, torch.zeros(2, 6, 4), torch.ones(1))), (K.pod_flat, (x[:, :, :1, :1], x[:, :, :1, :1]))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(*args)


# ---- kd_type validation ---------------------------------------------------------------------------------------------------------

def test_check_kd_type():
    from bdvcil_amd.cil_step import KD_TYPES, check_kd_type
    assert KD_TYPES == ('mse', 'pod', 'pod_spatial', 'pod_flat')
    assert check_kd_type('pod', 3) == ['pod'] * 3 and check_kd_type('mse', 0) == []
    assert check_kd_type(('pod_spatial', 'mse'), 2) == ['pod_spatial', 'mse']
    for bad, n in (('l2', 2), (None, 2), (['pod', 'cosine'], 2), (3, 1)):
        with pytest.raises(ValueError, match='kd_type'):
            check_kd_type(bad, n)
    with pytest.raises(ValueError, match='kd_type has 2 entries for 3'):
        check_kd_type(['pod', 'pod'], 3)


def _loop_config(**over):
    cfg = dict(work_dir='/nonexistent/never_created', task_splits=[[0, 1], [2, 3]], methods='base',
               kd_modules_names=['backbone.layer4', 'cls_head.avg_pool'], kd_weight_by_module=[0.5, 0.5], adaptive_scale_factors=[1.0, 1.4])
    cfg.update(over)
    return cfg


def _never(*a, **k):
    raise AssertionError('the clip loader must not be called')


def test_loop_validates_kd_type_before_any_file_or_gpu_work():
    """Every refusal below comes before the loop reads ``task_splits`` or builds a model: the config has no ``model`` key and a
    work_dir that cannot be created."""
    import bdvcil_amd as bd
    with pytest.raises(ValueError, match="kd_type='l2'"):
        bd.CILTaskLoop(_loop_config(kd_type='l2'), _never, device='cpu')
    with pytest.raises(ValueError, match='kd_type has 3 entries for 2'):
        bd.CILTaskLoop(_loop_config(kd_type=['pod', 'pod', 'pod']), _never, device='cpu')
    with pytest.raises(ValueError, match="kd_type='pod' has no effect with methods='icarl'"):
        bd.CILTaskLoop(_loop_config(kd_type='pod', methods='icarl'), _never, device='cpu')
    with pytest.raises(ValueError, match='kd_type'):
        bd.CILTaskLoop(_loop_config(kd_type=['pod_flat', 'pod_flat'], methods='icarl_video_mix'), _never, device='cpu')
    from bdvcil_amd.task_loop import check_loop_kd_type
    assert check_loop_kd_type(_loop_config()) == 'mse'                                   # absent = 'mse'
    assert check_loop_kd_type(_loop_config(kd_type='mse', methods='icarl')) == 'mse'     # the default is fine with any method
    assert check_loop_kd_type(_loop_config(kd_type=('pod_spatial', 'pod_flat'))) == ['pod_spatial', 'pod_flat']
    assert 'kd_type' in bd.CILTaskLoop.__doc__


def test_train_cil_flag():
    import tools.train_cil as T
    args = T.build_parser().parse_args(['cfg.py', '--kd-type', 'pod'])
    assert args.kd_type == 'pod' and T.build_parser().parse_args(['cfg.py']).kd_type is None
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['cfg.py', '--kd-type', 'l2'])
    import bdvcil_amd as bd
    assert tuple(bd.KD_TYPES) == T.KD_TYPES
