"""The conv entry points' argument checks, and the coverage of the bit-hash cases, on the host.

Refusals: every conv entry point is called through ``bd._lib.lib()`` with argument sets that each violate one condition (a NULL or
misaligned pointer, fields of ``bdv_conv_affine`` / ``bdv_bn_stat_fuse``, options that exclude each other, ``pieces`` out of range, a
slab that is too small, ...).  The pointers are made-up aligned addresses: the host never dereferences them, and every case is refused
before the first HIP call, so nothing here reaches a launch.  tests/golden/conv_launch_refusals.json holds, per case, the return
code and ``bdv_last_error()`` without its ``bdv_conv_...:`` prefix, recorded before the launch layer was rewritten
(``python tests/test_conv_launch_cpu.py`` re-records it).  The prefix may name any conv entry point: a call that enters through
``bdv_conv_fprop_f16x2`` may report as such or as the ``_pl`` call it shares its checks with.
(A ReLU mask with Cin % 32 != 0 cannot be reached as such: the data gradient needs Cin % 64 == 0, so the plan refuses first.)

Coverage: the kernels planned for the cases of tests/test_conv_bits_gpu.py (both lists) must include every kernel name of
tests/golden/conv_plan_sites.json, so that a launch layer that sent a plan to the wrong instantiation changes some hash."""
import ctypes
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (run as a script: re-recording)

import bdvcil_amd as bd
from bdvcil_amd import kernels as K
from bdvcil_amd._lib import BnStatFuse, ConvAffine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN = os.path.join(GOLDEN_DIR, 'conv_launch_refusals.json')

# arguments of each entry point, in the order of include/bdvcil_hip.h
ARGS = {
    'bdv_conv_fprop': ('x', 'w', 'y', 'geom', 'bn_partial', 'affine', 'workspace', 'workspace_bytes', 'stream'),
    'bdv_conv_fprop_pl': ('x', 'w', 'planes', 'y', 'geom', 'bn_partial', 'affine', 'workspace', 'workspace_bytes', 'pieces', 'pre_scale',
                          'pre_shift', 'stream'),
    'bdv_conv_fprop_f16x2': ('x', 'amax_x', 'w', 'planes', 'y', 'geom', 'bn_partial', 'affine', 'workspace', 'workspace_bytes',
                             'pre_scale', 'pre_shift', 'stream'),
    'bdv_conv_dgrad': ('dy', 'w', 'dx', 'add_src', 'add_mask_src', 'geom', 'bn_stat', 'workspace', 'workspace_bytes', 'stream'),
    'bdv_conv_dgrad_pl': ('dy', 'w', 'planes', 'dx', 'add_src', 'add_mask_src', 'geom', 'bn_stat', 'workspace', 'workspace_bytes',
                          'pieces', 'stream'),
    'bdv_conv_dgrad_f16x2': ('dy', 'amax_dy', 'w', 'planes', 'dx', 'add_src', 'add_mask_src', 'geom', 'bn_stat', 'workspace',
                             'workspace_bytes', 'stream'),
    'bdv_conv_wgrad': ('dy', 'x', 'dw', 'beta', 'geom', 'workspace', 'workspace_bytes', 'stream'),
    'bdv_conv_wgrad_partial': ('dy', 'x', 'geom', 'workspace', 'workspace_bytes', 'stream'),
    'bdv_conv_wgrad_partial_pl': ('dy', 'x', 'geom', 'workspace', 'workspace_bytes', 'pieces', 'pre_scale', 'pre_shift', 'stream'),
    'bdv_conv_wgrad_partial_f16x2': ('dy', 'amax_dy', 'x', 'amax_x', 'geom', 'workspace', 'workspace_bytes', 'pre_scale', 'pre_shift',
                                     'stream'),
}
FPROPS = ('bdv_conv_fprop', 'bdv_conv_fprop_pl', 'bdv_conv_fprop_f16x2')
DGRADS = ('bdv_conv_dgrad', 'bdv_conv_dgrad_pl', 'bdv_conv_dgrad_f16x2')
WGRADS = ('bdv_conv_wgrad', 'bdv_conv_wgrad_partial', 'bdv_conv_wgrad_partial_pl', 'bdv_conv_wgrad_partial_f16x2')
# the tensor pointers each entry point refuses as NULL / as misaligned, on a site of the plane kernels ('pl')
NONNULL = {
    'bdv_conv_fprop': ('x', 'w', 'y'), 'bdv_conv_fprop_pl': ('x', 'y'), 'bdv_conv_fprop_f16x2': ('x', 'y'),
    'bdv_conv_dgrad': ('dy', 'w', 'dx'), 'bdv_conv_dgrad_pl': ('dy', 'dx'), 'bdv_conv_dgrad_f16x2': ('dy', 'dx'),
    'bdv_conv_wgrad': ('dy', 'x', 'dw', 'workspace'), 'bdv_conv_wgrad_partial': ('dy', 'x', 'workspace'),
    'bdv_conv_wgrad_partial_pl': ('dy', 'x', 'workspace'), 'bdv_conv_wgrad_partial_f16x2': ('dy', 'x', 'workspace'),
}
ALIGNED = {
    'bdv_conv_fprop': ('x', 'w', 'y', 'workspace'), 'bdv_conv_fprop_pl': ('x', 'planes', 'y', 'workspace'),
    'bdv_conv_fprop_f16x2': ('x', 'planes', 'y', 'workspace'),
    'bdv_conv_dgrad': ('dy', 'w', 'dx', 'workspace'), 'bdv_conv_dgrad_pl': ('dy', 'planes', 'dx', 'workspace'),
    'bdv_conv_dgrad_f16x2': ('dy', 'planes', 'dx', 'workspace'),
    'bdv_conv_wgrad': ('dy', 'x', 'dw', 'workspace'), 'bdv_conv_wgrad_partial': ('dy', 'x', 'workspace'),
    'bdv_conv_wgrad_partial_pl': ('dy', 'x', 'workspace'), 'bdv_conv_wgrad_partial_f16x2': ('dy', 'x', 'workspace'),
}

# (N, H, W, Cin, Cout, R, S, stride, pad)
GEOMS = {
    'pl': (2, 14, 14, 128, 128, 3, 3, 1, 1),        # the plane kernels in every bf16-piece arithmetic; 128-wide fp32-MFMA kernels
    'x3': (2, 14, 14, 128, 128, 1, 1, 1, 0),        # short K: the two-workgroups-per-CU kernels, weights from the planes
    's2': (2, 14, 14, 128, 128, 1, 1, 2, 0),        # stride 2 behind a 1x1 filter: no fused statistics
    'stem': (2, 32, 32, 4, 64, 7, 7, 2, 3),
}
PTR_NAMES = ('x', 'w', 'y', 'dy', 'dx', 'dw', 'planes', 'workspace', 'amax_x', 'amax_dy', 'bn_partial', 'add_src', 'add_mask_src', 'pre_scale',
             'pre_shift', 'scale', 'shift', 'residual', 'bn_y', 'relu_mask', 'mean', 'invstd', 'partial', 'relu_scale', 'relu_shift')
ADDR = {n: 0x100000 * (i + 1) for i, n in enumerate(PTR_NAMES)}      # made-up, 16-byte aligned, never dereferenced
OFF4 = 4


def _affine(**kw):
    d = dict(scale=ADDR['scale'], shift=ADDR['shift'], residual=ADDR['residual'], relu=1)
    d.update(kw)
    return d


def _bn_stat(**kw):
    d = dict(y=ADDR['bn_y'], relu_mask=None, mean=ADDR['mean'], invstd=ADDR['invstd'], partial=ADDR['partial'], relu_scale=None,
             relu_shift=None)
    d.update(kw)
    return d


def _cases():
    """(id, entry point, geometry, the arguments that differ from a call that would be accepted)."""
    out = []
    for entry in ARGS:
        short = entry[len('bdv_conv_'):]
        for n in NONNULL[entry]:
            out.append((f'{short}/null-{n}', entry, 'pl', {n: None}))
        for n in ALIGNED[entry]:
            out.append((f'{short}/misaligned-{n}', entry, 'pl', {n: ADDR[n] + OFF4}))
    for entry in FPROPS:
        short = entry[len('bdv_conv_'):]
        out += [(f'{short}/stats-with-affine', entry, 'pl', dict(bn_partial=ADDR['bn_partial'], affine=_affine())),
                (f'{short}/affine-null-scale', entry, 'pl', dict(affine=_affine(scale=None))),
                (f'{short}/affine-null-shift', entry, 'pl', dict(affine=_affine(shift=None))),
                (f'{short}/affine-misaligned-shift', entry, 'pl', dict(affine=_affine(shift=ADDR['shift'] + OFF4))),
                (f'{short}/affine-misaligned-residual', entry, 'pl', dict(affine=_affine(residual=ADDR['residual'] + OFF4)))]
    for entry in DGRADS:
        short = entry[len('bdv_conv_'):]
        out += [(f'{short}/mask-without-add', entry, 'pl', dict(add_mask_src=ADDR['add_mask_src'])),
                (f'{short}/stat-null-mean', entry, 'pl', dict(bn_stat=_bn_stat(mean=None))),
                (f'{short}/stat-null-partial', entry, 'pl', dict(bn_stat=_bn_stat(partial=None))),
                (f'{short}/stat-misaligned-invstd', entry, 'pl', dict(bn_stat=_bn_stat(invstd=ADDR['invstd'] + OFF4))),
                (f'{short}/stat-misaligned-partial', entry, 'pl', dict(bn_stat=_bn_stat(partial=ADDR['partial'] + OFF4))),
                (f'{short}/stat-stride2-1x1', entry, 's2', dict(bn_stat=_bn_stat())),
                (f'{short}/relu-mask-cin4', entry, 'stem', dict(bn_stat=_bn_stat(relu_mask=ADDR['relu_mask'])))]
    out.append(('dgrad/relu-scale-128-wide-fp32', 'bdv_conv_dgrad', 'pl',
                dict(bn_stat=_bn_stat(relu_scale=ADDR['relu_scale'], relu_shift=ADDR['relu_shift']))))
    for entry in ('bdv_conv_fprop_pl', 'bdv_conv_fprop_f16x2', 'bdv_conv_wgrad_partial_pl', 'bdv_conv_wgrad_partial_f16x2'):
        out.append((f'{entry[len("bdv_conv_"):]}/pre-scale-without-shift', entry, 'x3', dict(pre_scale=ADDR['pre_scale'])))
    for entry in ('bdv_conv_fprop_pl', 'bdv_conv_fprop_f16x2'):
        short = entry[len('bdv_conv_'):]
        out += [(f'{short}/pre-misaligned-shift', entry, 'x3', dict(pre_scale=ADDR['pre_scale'], pre_shift=ADDR['pre_shift'] + OFF4)),
                (f'{short}/pre-misaligned-scale', entry, 'x3', dict(pre_scale=ADDR['pre_scale'] + OFF4, pre_shift=ADDR['pre_shift']))]
    for entry in ('bdv_conv_fprop_pl', 'bdv_conv_dgrad_pl', 'bdv_conv_wgrad_partial_pl'):
        out += [(f'{entry[len("bdv_conv_"):]}/pieces-{p}', entry, 'pl', dict(pieces=p)) for p in (0, 4, -1)]
    for entry in ('bdv_conv_fprop_pl', 'bdv_conv_fprop_f16x2', 'bdv_conv_dgrad_pl', 'bdv_conv_dgrad_f16x2'):
        short = entry[len('bdv_conv_'):]
        out += [(f'{short}/planes-null-plane-kernel', entry, 'pl', dict(planes=None)),
                (f'{short}/planes-null-x3-kernel', entry, 'x3', dict(planes=None))]
    for entry in ('bdv_conv_fprop_pl', 'bdv_conv_dgrad_pl'):        # a site of the conv_*_x3 kernels: the fp32-tensor checks apply
        short = entry[len('bdv_conv_'):]
        out += [(f'{short}/x3-null-w', entry, 'x3', dict(w=None)), (f'{short}/x3-misaligned-w', entry, 'x3', dict(w=ADDR['w'] + OFF4))]
    for entry in WGRADS:
        out.append((f'{entry[len("bdv_conv_"):]}/slab-too-small', entry, 'pl', dict(workspace_bytes=4096)))
    out += [('fprop_f16x2/null-amax', 'bdv_conv_fprop_f16x2', 'pl', dict(amax_x=None)),
            ('dgrad_f16x2/null-amax', 'bdv_conv_dgrad_f16x2', 'pl', dict(amax_dy=None)),
            ('wgrad_partial_f16x2/null-amax-dy', 'bdv_conv_wgrad_partial_f16x2', 'pl', dict(amax_dy=None)),
            ('wgrad_partial_f16x2/null-amax-x', 'bdv_conv_wgrad_partial_f16x2', 'pl', dict(amax_x=None))]
    return out


CASES = _cases()


def refusal(entry, geom, changed):
    """(return code, message without its prefix, prefix) of one call."""
    g = K.make_geom(*GEOMS[geom])
    g.act_dtype = 0
    args = {n: ADDR.get(n) for n in ARGS[entry]}
    args.update(geom=ctypes.byref(g), bn_partial=None, affine=None, bn_stat=None, add_src=None, add_mask_src=None, pre_scale=None,
                pre_shift=None, pieces=3, workspace_bytes=1 << 30, stream=None, beta=0.0)
    args.update(changed)
    keep = []
    if args.get('affine') is not None:
        a = args['affine']
        keep.append(ConvAffine(a['scale'], a['shift'], a['residual'], a['relu']))
        args['affine'] = ctypes.byref(keep[-1])
    if args.get('bn_stat') is not None:
        s = args['bn_stat']
        keep.append(BnStatFuse(s['y'], s['relu_mask'], s['mean'], s['invstd'], s['partial'], s['relu_scale'], s['relu_shift']))
        args['bn_stat'] = ctypes.byref(keep[-1])
    lib = bd._lib.lib()
    rc = getattr(lib, entry)(*[args[n] for n in ARGS[entry]])
    msg = lib.bdv_last_error().decode()
    m = re.match(r'(bdv_conv\w*): ', msg)
    return rc, (msg[m.end():] if m else msg), (m.group(1) if m else None)


def test_cases_cover_every_entry_point_and_the_golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(c[0] for c in CASES) and len({c[0] for c in CASES}) == len(CASES)
    assert {c[1] for c in CASES} == set(ARGS)
    for entry, names in ARGS.items():
        assert len(bd._lib.SIGNATURES[entry][1]) == len(names), entry
    assert {v[0] for v in want.values()} == {-1, -2}         # BDV_EINVAL and BDV_EWORKSPACE both occur


@pytest.mark.parametrize('cid,entry,geom,changed', CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, entry, geom, changed):
    with open(GOLDEN) as f:
        want = json.load(f)[cid]
    rc, text, prefix = refusal(entry, geom, changed)
    assert rc != 0 and [rc, text] == want
    # the prefix names a conv entry point (or the planner all of them share: "bdv_conv")
    assert prefix == 'bdv_conv' or prefix in ARGS, prefix


# ---- the bit-hash cases reach every kernel the dispatch can name ---------------------------------------------------------------

# kernel names of conv_plan_sites.json that no case of the two lists plans, each with its reason
UNREACHED = {}


def test_bit_cases_plan_every_kernel_of_the_plan_table():
    import test_conv_bits_gpu as B
    with open(os.path.join(GOLDEN_DIR, 'conv_plan_sites.json')) as f:
        names = set(json.load(f)['kernels'])
    with open(os.path.join(GOLDEN_DIR, 'conv_bits.json')) as f:
        old = json.load(f)
    with open(os.path.join(GOLDEN_DIR, 'conv_bits_launch.json')) as f:
        new = json.load(f)
    assert sorted(old) == sorted(B._key(*p) for p in B.PARAMS) and sorted(new) == sorted(B._launch_key(*p) for p in B.LAUNCH_PARAMS)
    planned = set()
    for si, mode, tile in B.PARAMS:
        planned |= set(B.planned_kernels(si, mode, tile, 'plain'))
    for p in B.LAUNCH_PARAMS:
        planned |= set(B.planned_kernels(*p))
    assert not (set(UNREACHED) - names) and not (set(UNREACHED) & planned)
    missing = sorted(names - planned - set(UNREACHED))
    assert not missing, f'no bit-hash case runs {missing}'


if __name__ == '__main__':
    table = {cid: list(refusal(entry, geom, changed)[:2]) for cid, entry, geom, changed in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + '\n}\n')
    print('wrote', len(table), 'cases')
