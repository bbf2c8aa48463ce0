"""``bdv_bn_eval_backward`` (backward through a BatchNorm that runs on its running statistics) against torch CPU.

``dy`` / ``dz`` are one select and one multiply per element: compared BIT for bit with the fp32 CPU expression
``(dout * [a > 0]) * scale`` (scale read back from the device's ``bn_eval_params``).  ``dgamma`` / ``dbeta`` are compared with an
fp64 evaluation of  dbeta = sum dz,  dgamma = sum dz * (y - running_mean) / sqrt(running_var + eps)  under the bars of
``tests/test_ops_gpu.py::test_bn_train_fwd_bwd``: max err <= 2e-5 * max|ref| + 1e-4 (2e-4 when accumulating onto a previous result).

Shapes: one row; fewer rows than one row block; ragged last row blocks; every branch of the supported channel counts (64, 128,
multiples of 256)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64), (7, 128), (1000, 64), (777, 128), (3000, 256), (130, 2048)]
SIGNS = ['mask', 'mask_res', 'act', 'none']
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _inputs(M, C):
    """CPU inputs of one shape, made once and shared (never modified)."""
    g = torch.Generator().manual_seed(1000 * C + M)
    y = torch.randn(M, C, generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) * 3.0 - 1.5              # uniform(-1.5, 1.5): negative channels are legal
    gamma[C // 3] = 0.0                                         # ... and so is a channel at exactly 0 (zero-initialised last BN)
    beta = torch.randn(C, generator=g) * 0.5
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) * 1.4 + 0.1                 # [0.1, 1.5]
    res = torch.randn(M, C, generator=g)
    dout = torch.randn(M, C, generator=g)
    return dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, res=res, dout=dout)


def _device_case(M, C, sign, dev, dtype=torch.float32):
    """-> (device operands for bn_eval_backward, CPU tensors the reference is formed from)."""
    from bdvcil_amd import kernels as K
    t = _inputs(M, C)
    d = {k: v.to(dev) for k, v in t.items()}
    scale, shift = K.bn_eval_params(d['gamma'], d['beta'], d['rm'], d['rv'], EPS)
    invstd = K.bn_eval_invstd(d['rv'], EPS)
    y, dout, res = d['y'].to(dtype), d['dout'].to(dtype), d['res'].to(dtype)
    kw, keep = {}, torch.ones(M, C, dtype=torch.bool)
    if sign != 'none':
        a, mask = K.bn_apply(y, scale, shift, res if sign == 'mask_res' else None, True, want_mask=True)
        keep = a.cpu().float() > 0
        kw = dict(relu_act=a) if sign == 'act' else dict(relu_mask=mask)
    ops = dict(dout=dout, scale=scale, y=y, running_mean=d['rm'], invstd=invstd, **kw)
    return ops, dict(keep=keep, scale=scale.cpu(), dout=dout.cpu().float(), y=y.cpu().float(), rm=t['rm'], rv=t['rv'])


def _reference(ref):
    zero = torch.zeros(())
    dz = torch.where(ref['keep'], ref['dout'], zero)            # fp32, exact
    dy = dz * ref['scale']                                      # one fp32 multiply: one rounding, nothing to contract
    dz64 = dz.double()
    xhat = (ref['y'].double() - ref['rm'].double()) / torch.sqrt(ref['rv'].double() + EPS)
    return dz, dy, (dz64 * xhat).sum(0), dz64.sum(0)


def _within(got, ref, atol):
    got, ref = got.cpu().double(), ref.double()
    assert torch.isfinite(got).all()
    err, bar = (got - ref).abs().max().item(), 2e-5 * ref.abs().max().item() + atol
    print(f'max err {err:.3e} (bar {bar:.3e})')
    assert err <= bar, (err, bar)


@pytest.mark.parametrize('sign', SIGNS)
@pytest.mark.parametrize('M,C', SHAPES)
def test_against_cpu(M, C, sign, dev):
    from bdvcil_amd import kernels as K
    ops, ref = _device_case(M, C, sign, dev)
    dz_ref, dy_ref, dg_ref, db_ref = _reference(ref)
    dy, dz, dg, db = K.bn_eval_backward(**ops, want_params=True, want_dz=True)
    assert torch.equal(dy.cpu(), dy_ref), (dy.cpu() - dy_ref).abs().max()
    assert torch.equal(dz.cpu(), dz_ref)
    _within(dg, dg_ref, 1e-4)
    _within(db, db_ref, 1e-4)
    zc = C // 3                                                 # the gamma = 0 channel: its dy is 0, its dgamma is not
    assert float(dy[:, zc].abs().max()) == 0.0 and bool(torch.isfinite(dg[zc]))
    assert abs(float(dg[zc]) - float(dg_ref[zc])) <= 2e-5 * dg_ref.abs().max().item() + 1e-4
    # without the optional second output the first one does not change
    dy1, none, dg1, db1 = K.bn_eval_backward(**ops, want_params=True)
    assert none is None and torch.equal(dy1, dy) and torch.equal(dg1, dg) and torch.equal(db1, db)
    # accumulate onto a previous result
    _, _, dg2, db2 = K.bn_eval_backward(**ops, dgamma=dg.clone(), dbeta=db.clone(), beta_acc=1.0)
    _within(dg2, 2 * dg_ref, 2e-4)
    _within(db2, 2 * db_ref, 2e-4)


@pytest.mark.parametrize('sign', SIGNS)
@pytest.mark.parametrize('M,C', SHAPES)
def test_without_parameter_gradients(M, C, sign, dev):
    """No y, no statistics, no workspace: the streaming form; dy (and dz) carry the bits of the form that also reduces."""
    from bdvcil_amd import kernels as K
    ops, ref = _device_case(M, C, sign, dev)
    dz_ref, dy_ref, _, _ = _reference(ref)
    slim = {k: v for k, v in ops.items() if k not in ('y', 'running_mean', 'invstd')}
    dy, dz, dg, db = K.bn_eval_backward(**slim, want_dz=True)
    assert dg is None and db is None
    assert torch.equal(dy.cpu(), dy_ref) and torch.equal(dz.cpu(), dz_ref)
    dy0 = K.bn_eval_backward(**slim)[0]
    assert torch.equal(dy0, dy)
    assert torch.equal(K.bn_eval_backward(**ops, want_params=True)[0], dy)


@pytest.mark.parametrize('sign', SIGNS)
def test_bf16_storage(sign, dev):
    """bf16 tensors (dout, activation, y, dy, dz): the fp32 product rounded once to bf16; sums stay fp32 / fp64."""
    from bdvcil_amd import kernels as K
    M, C = 777, 128
    ops, ref = _device_case(M, C, sign, dev, dtype=torch.bfloat16)
    dz_ref, dy_ref, dg_ref, db_ref = _reference(ref)
    for want_params in (True, False):
        use = ops if want_params else {k: v for k, v in ops.items() if k not in ('y', 'running_mean', 'invstd')}
        dy, dz, dg, db = K.bn_eval_backward(**use, want_params=want_params, want_dz=True)
        assert dy.dtype == torch.bfloat16 and dz.dtype == torch.bfloat16
        assert torch.equal(dy.cpu(), dy_ref.to(torch.bfloat16))
        assert torch.equal(dz.cpu(), dz_ref.to(torch.bfloat16))
        if want_params:
            _within(dg, dg_ref, 1e-4)
            _within(db, db_ref, 1e-4)


@pytest.mark.parametrize('M,C', [(777, 128), (3000, 256), (130, 2048)])
def test_parameter_gradients_are_deterministic(M, C, dev):
    """Two calls, and the one-block and the planner's finalize: the same bits."""
    from bdvcil_amd import kernels as K
    ops, _ = _device_case(M, C, 'mask_res', dev)
    runs = [K.bn_eval_backward(**ops, want_params=True, splits=s) for s in (0, 0, 1, 1)]
    for r in runs[1:]:
        assert torch.equal(r[2], runs[0][2]) and torch.equal(r[3], runs[0][3]) and torch.equal(r[0], runs[0][0])


def test_bad_input_is_an_error_not_a_launch(dev):
    from bdvcil_amd import kernels as K
    from bdvcil_amd._lib import HipExtensionError, check, lib
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())     # noqa: E731

    def call(M, C, dy=True, mask=False):
        dout = torch.zeros(M, C, device=dev)
        out = torch.zeros(M, C, device=dev) if dy else None
        scale = torch.ones(C, device=dev)
        m = torch.zeros(max(M * C // 32, 1), dtype=torch.int32, device=dev) if mask else None
        check(lib().bdv_bn_eval_backward(p(dout), p(m), None, None, p(scale), None, None, p(out), None, None, None, 0.0, M, C, None, 0,
                                         0, 0, None, 0, None), 'bdv_bn_eval_backward')
        torch.cuda.synchronize()
    call(8, 64)                                     # the harness itself is a valid call
    with pytest.raises(HipExtensionError, match='unsupported'):
        call(8, 96)
    with pytest.raises(HipExtensionError):
        call(8, 80, mask=True)                      # a mask needs C % 32 == 0; every C the BatchNorm kernels take is one, so this
                                                    # C is refused as unsupported before the mask check (kept behind it) is reached
    with pytest.raises(HipExtensionError, match='null'):
        call(8, 64, dy=False)
    with pytest.raises(HipExtensionError, match='unsupported'):
        K.bn_eval_backward(torch.zeros(8, 96, device=dev), torch.ones(96, device=dev))
    with pytest.raises(ValueError):                 # parameter gradients without y
        K.bn_eval_backward(torch.zeros(8, 64, device=dev), torch.ones(64, device=dev), want_params=True)
