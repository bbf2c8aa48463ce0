"""Host side of foreground merging (csrc/fg_merge.hip, ``ForegroundMergeBlending``, the loop's ``fg_merge`` key; no device needed): the
C ABI of the four entry points and their refusals (on their arguments, before any launch), the wrappers' refusals, the registry, the
draws, ``check_loop_fg_merge``, the CLI flags, and the torch restatement of the chain (tests/fg_merge_oracle.py) on the two-halves
scene in fp32 and fp64."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import bdvcil_amd as bd
import fg_merge_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'bdv_fg_motion_q': 15, 'bdv_fg_hist_refine': 15, 'bdv_fg_select': 8, 'bdv_fg_merge': 15}
K = bd.kernels

ONE = ctypes.c_void_p(16)         # aligned, never dereferenced: every call below is refused on its arguments
NULL = ctypes.c_void_p(0)
TAPS = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
TRIPLE = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

TWO_HALVES = [(2, 3, 20, 20), (2, 4, 12, 18), (2, 2, 16, 24), (1, 8, 224, 224)]
MOTION_SHAPES = [(3, 3, 20, 20), (2, 4, 13, 19), (2, 2, 16, 24), (1, 8, 224, 224)]      # the shapes of the GPU file


def _lib():
    return bd._lib.lib()


def _refused(rc, name):
    msg = _lib().bdv_last_error()
    assert rc == -1 and msg.startswith(name.encode()), (rc, msg)
    return msg.decode()


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')) as f:
        header = f.read()
    raw = ctypes.CDLL(bd._lib.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int ' + name + r'\s*\(', header, re.S)
        assert m and 'beyond the reference' in m.group(1), name
        assert len(bd._lib.SIGNATURES[name][1]) == nargs and hasattr(raw, name)
        decl = header[header.index('int ' + name + '('):]
        assert decl[:decl.index(';')].count(',') + 1 == nargs, name
    assert 'fg_merge.hip' in bd._lib.HASHED_SOURCES
    mk = open(os.path.join(ROOT, 'background-debiased-video-cil_amd', 'csrc', 'Makefile')).read()
    contract = [l for l in mk.splitlines() if '-ffp-contract=off' in l]
    assert 'fg_merge.hip' in mk and any('fg_merge.o' in l for l in contract)
    for fn in ('fg_motion_q', 'fg_hist_refine', 'fg_select', 'fg_merge_', 'fg_blur_taps', 'fg_colour_params'):
        assert hasattr(K, fn)
    for fn in ('ForegroundMergeBlending', 'foreground_mask'):
        assert hasattr(bd, fn)
    assert 'PARITY UNPINNED' in bd.ForegroundMergeBlending.__doc__ and 'PARITY UNPINNED' in bd.foreground_mask.__doc__


def test_motion_q_refusals():
    f, name = _lib().bdv_fg_motion_q, 'bdv_fg_motion_q'
    good = [ONE, 2, 3, 20, 20, 0, TAPS, 3, ONE, ONE, ONE, ONE, ONE, ONE, None]
    for i in (0, 6, 8, 9, 10, 11, 12, 13):
        a = list(good)
        a[i] = NULL
        assert 'null pointer' in _refused(f(*a), name)
    for i, v in ((1, 0), (1, 65536), (2, 0), (3, 0), (4, -1), (3, 1 << 13), (5, 3), (5, -1), (7, 0), (7, 2), (7, 131), (7, 41), (2, 1)):
        a = list(good)
        a[i] = v
        if i == 3 and v == 1 << 13:
            a[4] = 1 << 13                  # H * W = 2^26
        _refused(f(*a), name)
    a = list(good)
    a[0] = ctypes.c_void_p(18)
    assert 'alignment' in _refused(f(*a), name)


def test_hist_refine_refusals():
    f, name = _lib().bdv_fg_hist_refine, 'bdv_fg_hist_refine'
    good = [ONE, ONE, 2, 3, 20, 20, 0, 8, TRIPLE, TRIPLE, ONE, ONE, ONE, ONE, None]
    for i in (0, 1, 8, 9, 10, 11, 12, 13):
        a = list(good)
        a[i] = NULL
        assert 'null pointer' in _refused(f(*a), name)
    for bins in (1, 0, 17, -8):
        a = list(good)
        a[7] = bins
        assert 'bins' in _refused(f(*a), name)
    a = list(good)
    a[3], a[4], a[5] = 8, 1500, 1500          # 255 * 18e6 >= 2^32, every other bound respected
    assert 'uint32' in _refused(f(*a), name)
    a[3] = 7                                   # 255 * 15.75e6 < 2^32: passes that check and is refused further on (alignment of idx)
    a[10] = ctypes.c_void_p(12)
    assert 'alignment' in _refused(f(*a), name)
    for i, v in ((2, 0), (6, 5), (3, 0)):
        a = list(good)
        a[i] = v
        _refused(f(*a), name)


def test_select_and_merge_refusals():
    f, name = _lib().bdv_fg_select, 'bdv_fg_select'
    good = [ONE, 2, 400, 200, ONE, ONE, ONE, None]
    for i in (0, 4, 5, 6):
        a = list(good)
        a[i] = NULL
        assert 'null pointer' in _refused(f(*a), name)
    for i, v in ((1, 0), (2, 0), (2, (1 << 24) + 1), (3, 0), (3, 401), (3, -5)):
        a = list(good)
        a[i] = v
        _refused(f(*a), name)
    f, name = _lib().bdv_fg_merge, 'bdv_fg_merge'
    good = [ONE, ONE, ONE, ONE, ONE, ONE, 2, 3, 3, 20, 20, 0, ONE, 1 << 30, None]
    for i in (0, 1, 2, 3, 4, 5):
        a = list(good)
        a[i] = NULL
        assert 'null pointer' in _refused(f(*a), name)
    a = list(good)
    a[12] = NULL
    assert 'null scratch' in _refused(f(*a), name)
    a = list(good)
    a[13] = 2 * 3 * 3 * 400 * 4 - 1            # one byte short of two slots
    assert 'scratch' in _refused(f(*a), name)
    for i, v in ((6, 4), (6, -1), (7, 0), (8, 0), (11, 7), (12, ctypes.c_void_p(8))):
        a = list(good)
        a[i] = v
        _refused(f(*a), name)


def test_wrappers_refuse_before_touching_the_device():
    x = torch.zeros(2, 3, 3, 20, 20)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.fg_motion_q(x, 2, 3, 20, 20)
    with pytest.raises(ValueError, match='two frames'):
        K.fg_motion_q(x[:, :1].contiguous(), 2, 1, 20, 20)
    with pytest.raises(ValueError, match='not a batch'):
        K.fg_motion_q(x, 2, 3, 20, 21)
    with pytest.raises(ValueError, match='layout'):
        K.fg_motion_q(x, 2, 3, 20, 20, layout='nchw')
    q = torch.zeros(2, 20, 20, dtype=torch.uint8)
    lo, sc = K.fg_colour_params(8, FO.IMG_MEAN, FO.IMG_STD)
    for bins in (1, 17, 2.5, True):
        with pytest.raises(ValueError, match='bins'):
            K.fg_hist_refine(x, q, 2, 3, 20, 20, 'tchw', bins, lo, sc)
    with pytest.raises(ValueError, match='uint32'):
        K.fg_hist_refine(x, q, 2, 8, 1500, 1500, 'tchw', 8, lo, sc)
    with pytest.raises(ValueError, match='q '):
        K.fg_hist_refine(x, q[:, :19], 2, 3, 20, 20, 'tchw', 8, lo, sc)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.fg_hist_refine(x, q, 2, 3, 20, 20, 'tchw', 8, lo, sc)
    for beta in (0, -0.1, 1.0001, 'half', None, True):
        with pytest.raises(ValueError, match='beta'):
            bd.foreground_mask(x, beta=beta)
        with pytest.raises(ValueError, match='beta'):
            bd.ForegroundMergeBlending(beta=beta)
    assert K.fg_k_fg(1.0, 20, 20) == 400 and K.fg_k_fg(0.5, 13, 19) == 123 and K.fg_k_fg(1e-9, 20, 20) == 1
    with pytest.raises(ValueError, match='k_fg'):
        K.fg_select(torch.zeros(2, 400), 401)
    mask = torch.zeros(2, 20, 20, dtype=torch.uint8)
    count = torch.zeros(2, dtype=torch.int32)
    perm, apply = torch.tensor([1, 0]), torch.tensor([True, True])
    with pytest.raises(ValueError, match='mask'):              # mask and clip shapes that disagree
        K.fg_merge_(x, mask[:, :, :19], count, perm, apply, 2, 3, 20, 20)
    with pytest.raises(ValueError, match='mask'):
        K.fg_merge_(x, torch.zeros(3, 20, 20, dtype=torch.uint8), count, perm, apply, 2, 3, 20, 20)
    with pytest.raises(ValueError, match='not a batch'):
        K.fg_merge_(x, mask, count, perm, apply, 2, 3, 20, 20, layout='thwc4')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.fg_merge_(x, mask, count, perm, apply, 2, 3, 20, 20)
    with pytest.raises(ValueError):
        bd.foreground_mask(torch.zeros(2, 3, 20, 20))
    for mean, std in (((1, 2), FO.IMG_STD), (FO.IMG_MEAN, (1, 0, 1))):
        with pytest.raises(ValueError, match='mean and std'):
            bd.foreground_mask(x, mean=mean, std=std)


def test_host_parameters_match_the_restatement():
    for H, W, k in ((224, 224, 23), (20, 20, 3), (19, 40, 1), (13, 19, 1), (16, 24, 1), (64, 48, 5)):
        taps = K.fg_blur_taps(H, W)
        assert taps.numel() == k == FO.tap_count(H, W) and taps.dtype == torch.float32 and torch.equal(taps, FO.blur_taps(H, W))
        assert abs(taps.double().sum().item() - 1) < 1e-6
    assert K.fg_blur_taps(16, 16).tolist() == [1.0]
    for bins in (2, 8, 16):
        lo, sc = K.fg_colour_params(bins, FO.IMG_MEAN, FO.IMG_STD)
        rlo, rsc = FO.colour_params(bins)
        assert torch.equal(lo, rlo) and torch.equal(sc, rsc) and lo.dtype == torch.float32
    slot, n = K.fg_merge_slots(torch.tensor([0, 2, 1, 4, 5, 3]), torch.tensor([True, True, True, True, False, True]))
    # 0: fixed point; 1 <-> 2 both merged: both staged; 3 <- 4 (4 stays: read directly); 4 off; 5 <- 3 (3 is merged: staged)
    assert slot.tolist() == [-1, 0, 1, -1, -1, 2] and n == 3


def test_registry_builds_the_blending():
    assert 'ForegroundMergeBlending' in bd.BLENDINGS
    b = bd.build_blending(dict(type='ForegroundMergeBlending'))
    assert (b.beta, b.prob, b.bins) == (0.5, 0.5, 8) and b.mean == tuple(bd.frontend.IMG_MEAN) and b.std == tuple(bd.frontend.IMG_STD)
    b = bd.build_blending(dict(type='ForegroundMergeBlending', beta=0.3, prob=1.0, bins=4, num_classes=101))
    assert (b.beta, b.prob, b.bins, b.num_classes) == (0.3, 1.0, 4, 101)
    for bad in (dict(prob=-0.1), dict(prob=1.5), dict(bins=1), dict(bins=17), dict(beta=0)):
        with pytest.raises(ValueError):
            bd.build_blending(dict(type='ForegroundMergeBlending', **bad))
    from oracle import tsm_oracle as O
    cfg = O.r50_cfg(num_classes=7, depth=18)
    cfg['train_cfg'] = dict(blending=dict(type='ForegroundMergeBlending', prob=0.25))
    assert isinstance(bd.build_model(cfg).blending, bd.ForegroundMergeBlending)


@pytest.mark.parametrize('seed', range(4))
def test_draw_is_reproducible_in_the_stated_order(seed):
    B = 6
    torch.manual_seed(seed)
    perm = torch.randperm(B)
    apply = torch.rand(B) < 0.4
    after = torch.rand(1)
    torch.manual_seed(seed)
    p, a = bd.ForegroundMergeBlending(prob=0.4).draw(B, 20, 20)
    assert torch.equal(p, perm) and torch.equal(a, apply) and a.dtype == torch.bool and torch.equal(torch.rand(1), after)


def test_cases_that_launch_nothing_return_the_object():
    lab = torch.tensor([[1], [2], [3]])
    for imgs, blend in ((torch.zeros(3, 1, 3, 20, 20), bd.ForegroundMergeBlending(prob=1.0)),        # T < 2
                        (torch.zeros(1, 3, 3, 20, 20), bd.ForegroundMergeBlending(prob=1.0)),        # B == 1
                        (torch.zeros(3, 3, 3, 20, 20), bd.ForegroundMergeBlending(prob=0))):         # prob == 0
        torch.manual_seed(3)
        after = torch.rand(1)
        torch.manual_seed(3)
        out, l = blend(imgs, lab[:imgs.shape[0]])               # host tensors: any launch would raise
        assert out is imgs and l.data_ptr() == lab.data_ptr() and torch.equal(torch.rand(1), after)      # and nothing was drawn


def test_check_loop_fg_merge():
    chk = bd.task_loop.check_loop_fg_merge
    assert chk({}) is None and chk({'fg_merge': None}) is None
    assert chk({'fg_merge': {}}) == dict(beta=0.5, prob=0.5, bins=8)
    assert chk({'fg_merge': dict(beta=1, prob=0, bins=16)}) == dict(beta=1, prob=0, bins=16)
    for bad in (dict(alpha=1), dict(beta=0), dict(beta=1.5), dict(beta='x'), dict(prob=-0.5), dict(prob=2), dict(bins=1), dict(bins=17),
                dict(bins=8.0), dict(prob=True), 0.5, [0.5]):
        with pytest.raises(ValueError, match='fg_merge'):
            chk({'fg_merge': bad})


def test_cli_flags_set_the_key():
    spec = importlib.util.spec_from_file_location('train_cil_cli', os.path.join(ROOT, 'tools', 'train_cil.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    a = ap.parse_args(['cfg.py'])
    assert a.fg_merge_prob is None and a.fg_merge_beta is None and 'fg_merge' not in cli.set_fg_merge({}, None, None)
    a = ap.parse_args(['cfg.py', '--fg-merge-prob', '0.3'])
    assert cli.set_fg_merge({}, a.fg_merge_prob, a.fg_merge_beta) == {'fg_merge': {'prob': 0.3}}
    a = ap.parse_args(['cfg.py', '--fg-merge-prob', '0.3', '--fg-merge-beta', '0.25'])
    cfg = cli.set_fg_merge({'fg_merge': dict(prob=0.9, bins=4)}, a.fg_merge_prob, a.fg_merge_beta)
    assert cfg['fg_merge'] == dict(prob=0.3, bins=4, beta=0.25) and bd.task_loop.check_loop_fg_merge(cfg) == dict(beta=0.25, prob=0.3, bins=4)
    assert cli.set_fg_merge({'fg_merge': dict(prob=0.9)}, None, 0.75)['fg_merge'] == dict(prob=0.9, beta=0.75)
    with pytest.raises(SystemExit):
        cli.set_fg_merge({}, None, 0.75)
    with pytest.raises(ValueError, match='fg_merge'):
        bd.task_loop.check_loop_fg_merge(cli.set_fg_merge({}, 1.5, None))


# ---- the restatement itself -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', TWO_HALVES, ids=str)
def test_oracle_two_halves_scene(shape):
    B, T, H, W = shape
    x = FO.two_halves_scene(*shape, seed=sum(shape))
    left = torch.zeros((B, H, W), dtype=torch.uint8)
    left[..., :W // 2] = 1
    out = {}
    for dtype in (torch.float32, torch.float64):
        s, mask, count, q = FO.foreground_mask(x, beta=0.5, dtype=dtype)
        assert s.dtype == dtype and torch.equal(mask, left) and count.tolist() == [H * (W // 2)] * B
        assert s[..., :W // 2].min() > s[..., W // 2:].max()
        out[dtype] = (s, q)
    dq = (out[torch.float32][1].int() - out[torch.float64][1].int()).abs()
    assert dq.max() <= 1 and (dq > 0).float().mean() <= 1e-3
    if int(dq.max()) == 0:                      # equal q: equal histograms, and s differs by its own rounding only
        assert (out[torch.float32][0].double() - out[torch.float64][0]).abs().max() <= (T + 6) * 2.0 ** -24


def test_oracle_static_clip_has_no_foreground():
    x = FO.two_halves_scene(2, 3, 20, 20)[:, :1].repeat(1, 3, 1, 1, 1)
    for dtype in (torch.float32, torch.float64):
        s, mask, count, q = FO.foreground_mask(x, dtype=dtype)
        assert count.tolist() == [0, 0] and not mask.any() and not q.any() and not s.any()


@pytest.mark.parametrize('i', range(len(MOTION_SHAPES)), ids=[str(s) for s in MOTION_SHAPES])
def test_fp32_oracle_stays_under_a_tenth_of_the_q_cap(i):
    """The GPU test allows q to differ from the fp64 oracle's by 1 at up to 1 % of the pixels; the fp32 restatement, which rounds as
    the kernels do, must itself stay under a tenth of that on the same inputs."""
    x = FO.random_clip(*MOTION_SHAPES[i], seed=i)
    q64, g64, _ = FO.motion_q(x, torch.float64)
    q32, g32, _ = FO.motion_q(x, torch.float32)
    dq = (q32.int() - q64.int()).abs()
    assert dq.max() <= 1 and (dq > 0).float().mean() <= 1e-3
    T, k = MOTION_SHAPES[i][1], FO.tap_count(*MOTION_SHAPES[i][2:])
    assert ((g32.double() - g64).abs() <= (3 * (T - 1) + 2 * k + 8) * 2.0 ** -24 * g64).all()
    assert q64.max() == 255 and q64.min() == 0


def test_oracle_merge_is_gather_then_assign():
    x = torch.arange(3 * 2 * 3 * 2 * 2, dtype=torch.float32).view(3, 2, 3, 2, 2)
    mask = torch.tensor([[[1, 0], [0, 0]], [[0, 1], [0, 0]], [[1, 1], [1, 1]]], dtype=torch.uint8)
    out = FO.merge(x, mask, torch.tensor([1, 1, 1]), torch.tensor([1, 0, 2]), torch.tensor([True, True, True]))
    assert torch.equal(out[0, :, :, 0, 0], x[0, :, :, 0, 0]) and torch.equal(out[0, :, :, 1, 1], x[1, :, :, 1, 1])
    assert torch.equal(out[1, :, :, 0, 1], x[1, :, :, 0, 1]) and torch.equal(out[1, :, :, 0, 0], x[0, :, :, 0, 0])      # x[0] as it WAS
    assert torch.equal(out[2], x[2])
