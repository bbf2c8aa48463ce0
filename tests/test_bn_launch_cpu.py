"""The argument checks of every entry point of csrc/bn.hip, on the host.

Each entry point is called through ``bd._lib.lib()`` with argument sets that each violate exactly one condition (a ``BDV_REQUIRE``, a
workspace size, a condition of ``bn_fin_resolve``).  The pointers are made-up aligned addresses: the host never dereferences them, and
every case is refused before the first HIP call, so nothing here reaches a launch.  tests/golden/bn_launch_refusals.json holds, per
case, the return code and ``bdv_last_error()``, recorded before the launch layer of bn.hip was rewritten
(``python tests/test_bn_launch_cpu.py`` re-records it).

What tests/test_frozen_bn_cpu.py (seven refusals of ``bdv_bn_eval_backward``) and tests/test_bn_chain_cpu.py (``splits`` = 3 and a split
without scratch in ``bdv_bn_train_finalize_split``) pin is not repeated here.

Conditions that cannot be violated alone, and are therefore left out:
  * "bf16 tensors need C % 8 == 0" of bdv_bn_backward, bdv_bn_backward_pair and bdv_bn_eval_backward, "relu needs ... C % 32 == 0" of
    bdv_bn_backward with a mask, C % 32 of bdv_bn_backward_pair and "relu_mask needs C % 32 == 0" of bdv_bn_eval_backward: these entry
    points accept C = 64, 128 or a multiple of 256 only, and the shape check refuses every other C with its own message;
  * C % 4 != 0 in ``bn_fin_resolve``: every caller has refused such a C before;
  * "tensor too large" of bdv_bn_backward_pair: the parent made this check after its first launches, so no host-only call reached it
    when the golden was recorded."""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (run as a script: re-recording)

import bdvcil_amd as bd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bn_launch_refusals.json')

# arguments of each entry point, in the order of include/bdvcil_hip.h
_FIN = ('splits', 'fin_scratch', 'fin_scratch_bytes')
_BWD = ('dout', 'relu_mask', 'y', 'gamma', 'save_mean', 'save_invstd', 'dy', 'dgamma', 'dbeta', 'beta_acc', 'M', 'C', 'relu', 'stat_partial',
        'stat_rows', 'relu_scale', 'relu_shift', 'workspace', 'workspace_bytes', 'act_dtype')
_POOL = ('dpool', 'pool_idx', 'relu_mask', 'y', 'gamma', 'save_mean', 'save_invstd', 'dy', 'dgamma', 'dbeta', 'beta_acc', 'N', 'H', 'W', 'C',
         'workspace', 'workspace_bytes', 'act_dtype')
_TRAIN_FIN = ('partial', 'rows', 'M', 'C', 'gamma', 'beta', 'eps', 'momentum', 'running_mean', 'running_var', 'save_mean', 'save_invstd',
              'scale', 'shift')
ARGS = {
    'bdv_bn_train_stats': ('y', 'M', 'C', 'gamma', 'beta', 'eps', 'momentum', 'running_mean', 'running_var', 'save_mean', 'save_invstd',
                           'scale', 'shift', 'workspace', 'workspace_bytes', 'stream'),
    'bdv_bn_train_finalize_split': _TRAIN_FIN + _FIN + ('stream',),
    'bdv_bn_train_finalize': _TRAIN_FIN + ('stream',),
    'bdv_bn_eval_params': ('C', 'gamma', 'beta', 'running_mean', 'running_var', 'eps', 'scale', 'shift', 'stream'),
    'bdv_bn_apply': ('y', 'scale', 'shift', 'res', 'res_scale', 'res_shift', 'out', 'relu_mask', 'M', 'C', 'relu', 'act_dtype', 'stream'),
    'bdv_bn_backward_split': _BWD + _FIN + ('stream',),
    'bdv_bn_backward': _BWD + ('stream',),
    'bdv_bn_backward_pair': ('dout', 'relu_mask', 'ya', 'gamma_a', 'mean_a', 'invstd_a', 'stat_partial', 'stat_rows', 'dya', 'dgamma_a',
                             'dbeta_a', 'yb', 'gamma_b', 'mean_b', 'invstd_b', 'dyb', 'dgamma_b', 'dbeta_b', 'M', 'C', 'workspace',
                             'workspace_bytes', 'act_dtype') + _FIN + ('stream',),
    'bdv_bn_eval_backward': ('dout', 'relu_mask', 'relu_act', 'y', 'scale', 'running_mean', 'invstd', 'dy', 'dz', 'dgamma', 'dbeta', 'beta_acc',
                             'M', 'C', 'workspace', 'workspace_bytes', 'act_dtype') + _FIN + ('stream',),
    'bdv_bn_backward_maxpool_split': _POOL + _FIN + ('stream',),
    'bdv_bn_backward_maxpool': _POOL + ('stream',),
    'bdv_relu_bwd': ('dout', 'relu_mask', 'add', 'g', 'numel', 'act_dtype', 'stream'),
    'bdv_add': ('a', 'b', 'out', 'numel', 'act_dtype', 'stream'),
}
SCALARS = dict(M=37, C=64, N=2, H=8, W=10, rows=8, eps=1e-5, momentum=0.1, beta_acc=0.0, relu=1, act_dtype=0, stat_rows=0, splits=1,
               fin_scratch_bytes=0, workspace_bytes=1 << 30, numel=64, stream=None)
PTR_NAMES = sorted({n for names in ARGS.values() for n in names} - set(SCALARS))
ADDR = {n: 0x100000 * (i + 1) for i, n in enumerate(PTR_NAMES)}      # made-up, 16-byte aligned, distinct, never dereferenced
OFF4, OFF1 = 4, 1
# pointers that an accepted call may leave NULL, and does in the base call of each case
OPTIONAL = ('running_mean', 'running_var', 'res', 'res_scale', 'res_shift', 'stat_partial', 'relu_scale', 'relu_shift', 'fin_scratch', 'add',
            'relu_act', 'dz')
BASE = {      # per entry point: what differs from SCALARS / ADDR in the call that would be accepted
    'bdv_bn_eval_backward': dict(y=None, running_mean=None, invstd=None, dgamma=None, dbeta=None, workspace=None, workspace_bytes=0),
}
EVAL_STATS = dict(y=ADDR['y'], running_mean=ADDR['running_mean'], invstd=ADDR['invstd'], dgamma=ADDR['dgamma'], dbeta=ADDR['dbeta'],
                  workspace=ADDR['workspace'], workspace_bytes=1 << 30)      # bdv_bn_eval_backward with parameter gradients

NONNULL = {
    'bdv_bn_train_stats': ('y', 'gamma', 'beta', 'save_mean', 'save_invstd', 'scale', 'shift', 'workspace'),
    'bdv_bn_train_finalize_split': ('partial', 'gamma', 'beta', 'save_mean', 'save_invstd', 'scale', 'shift'),
    'bdv_bn_train_finalize': ('partial',),
    'bdv_bn_eval_params': ('gamma', 'beta', 'running_mean', 'running_var', 'scale', 'shift'),
    'bdv_bn_apply': ('y', 'scale', 'shift', 'out'),
    'bdv_bn_backward_split': ('dout', 'y', 'gamma', 'save_mean', 'save_invstd', 'dy', 'workspace'),
    'bdv_bn_backward': ('dout',),
    'bdv_bn_backward_pair': ('dout', 'relu_mask', 'ya', 'gamma_a', 'mean_a', 'invstd_a', 'dya', 'yb', 'gamma_b', 'mean_b', 'invstd_b', 'dyb',
                             'workspace'),
    'bdv_bn_eval_backward': ('dout', 'scale'),
    'bdv_bn_backward_maxpool_split': ('dpool', 'pool_idx', 'relu_mask', 'y', 'gamma', 'save_mean', 'save_invstd', 'dy', 'workspace'),
    'bdv_bn_backward_maxpool': ('dpool',),
    'bdv_relu_bwd': ('dout', 'relu_mask', 'g'),
    'bdv_add': ('a', 'b', 'out'),
}
ALIGNED = {
    'bdv_bn_train_stats': ('y', 'workspace'),
    'bdv_bn_apply': ('y', 'out', 'scale', 'shift'),
    'bdv_bn_backward_split': ('dout', 'y', 'dy', 'workspace', 'save_mean', 'save_invstd'),
    'bdv_bn_backward_pair': ('dout', 'ya', 'yb', 'dya', 'dyb', 'workspace', 'mean_a', 'invstd_a', 'mean_b', 'invstd_b'),
    'bdv_bn_eval_backward': ('dout', 'scale'),
    'bdv_bn_backward_maxpool_split': ('dpool', 'y', 'dy', 'workspace', 'save_mean', 'save_invstd'),
    'bdv_relu_bwd': ('dout', 'g'),
    'bdv_add': ('a', 'b', 'out'),
}
# the entry points whose checks end in bn_fin_resolve (bdv_bn_train_finalize_split: tests/test_bn_chain_cpu.py has the first two)
FIN_RESOLVE = ('bdv_bn_backward_split', 'bdv_bn_backward_pair', 'bdv_bn_eval_backward', 'bdv_bn_backward_maxpool_split')


def _cases():
    """(id, entry point, the arguments that differ from a call that would be accepted)."""
    out = []
    add = lambda cid, entry, **changed: out.append((f'{entry[len("bdv_"):]}/{cid}', entry, changed))      # noqa: E731
    for entry, names in NONNULL.items():
        for n in names:
            add(f'null-{n}', entry, **{n: None})
    for entry, names in ALIGNED.items():
        for n in names:
            add(f'misaligned-{n}', entry, **{n: ADDR[n] + OFF4})
    for entry in ARGS:
        if 'act_dtype' in ARGS[entry] and entry not in ('bdv_bn_eval_backward', 'bdv_bn_backward', 'bdv_bn_backward_maxpool'):
            add('act-dtype-7', entry, act_dtype=7)
    for entry in FIN_RESOLVE:
        stats = EVAL_STATS if entry == 'bdv_bn_eval_backward' else {}
        add('splits-3', entry, splits=3, **stats)
        add('split-without-scratch', entry, splits=4, **stats)
    for entry in ('bdv_bn_train_stats', 'bdv_bn_backward_split', 'bdv_bn_backward', 'bdv_bn_backward_pair', 'bdv_bn_backward_maxpool_split'):
        add('workspace-too-small', entry, workspace_bytes=4096)
    for entry in ('bdv_bn_train_stats', 'bdv_bn_backward_split', 'bdv_bn_backward_pair'):
        add('M-0', entry, M=0)
        add('C-96', entry, C=96)
    add('M-0', 'bdv_bn_eval_backward', M=0)
    # running statistics come in pairs
    for entry in ('bdv_bn_train_stats', 'bdv_bn_train_finalize_split'):
        add('running-mean-alone', entry, running_mean=ADDR['running_mean'])
        add('running-var-alone', entry, running_var=ADDR['running_var'])
    # bdv_bn_train_finalize(_split): shape, and the conditions of bn_fin_resolve that test_bn_chain_cpu.py leaves
    for k, v in (('rows', 0), ('M', 0), ('C', 0), ('C', 66)):
        add(f'{k}-{v}', 'bdv_bn_train_finalize_split', **{k: v})
    add('rows-0', 'bdv_bn_train_finalize', rows=0)
    scratch = dict(fin_scratch=ADDR['fin_scratch'], fin_scratch_bytes=1 << 24)
    add('scratch-misaligned', 'bdv_bn_train_finalize_split', splits=2, fin_scratch=ADDR['fin_scratch'] + OFF4, fin_scratch_bytes=1 << 24)
    add('scratch-too-small', 'bdv_bn_train_finalize_split', splits=2, fin_scratch=ADDR['fin_scratch'], fin_scratch_bytes=4096 + 64 * 256 - 1)
    add('split-C-4100', 'bdv_bn_train_finalize_split', splits=2, C=4100, **scratch)
    add('split-C-4352', 'bdv_bn_backward_split', splits=2, C=4352, **scratch)
    add('C-0', 'bdv_bn_eval_params', C=0)
    # bdv_bn_apply
    res = dict(res=ADDR['res'])
    add('res-scale-without-shift', 'bdv_bn_apply', res_scale=ADDR['res_scale'], **res)
    add('res-shift-without-scale', 'bdv_bn_apply', res_shift=ADDR['res_shift'], **res)
    add('res-affine-without-res', 'bdv_bn_apply', res_scale=ADDR['res_scale'], res_shift=ADDR['res_shift'])
    add('misaligned-res-scale', 'bdv_bn_apply', res_scale=ADDR['res_scale'] + OFF4, res_shift=ADDR['res_shift'], **res)
    add('misaligned-res-shift', 'bdv_bn_apply', res_scale=ADDR['res_scale'], res_shift=ADDR['res_shift'] + OFF4, **res)
    add('misaligned-res', 'bdv_bn_apply', res=ADDR['res'] + OFF4)
    for k, v in (('M', 0), ('C', 0), ('C', 66)):
        add(f'{k}-{v}', 'bdv_bn_apply', relu_mask=None, **{k: v})
    add('mask-without-relu', 'bdv_bn_apply', relu=0)
    add('mask-C-36', 'bdv_bn_apply', C=36)
    add('bf16-C-36', 'bdv_bn_apply', C=36, act_dtype=1, relu_mask=None)
    # bdv_bn_backward_split
    add('stat-partial-rows-0', 'bdv_bn_backward_split', stat_partial=ADDR['stat_partial'])
    add('stat-partial-misaligned', 'bdv_bn_backward_split', stat_partial=ADDR['stat_partial'] + OFF4, stat_rows=3)
    add('relu-without-sign-source', 'bdv_bn_backward_split', relu_mask=None)
    add('relu-scale-without-shift', 'bdv_bn_backward_split', relu_mask=None, relu_scale=ADDR['relu_scale'])
    add('misaligned-relu-scale', 'bdv_bn_backward_split', relu_mask=None, relu_scale=ADDR['relu_scale'] + OFF4, relu_shift=ADDR['relu_shift'])
    add('misaligned-relu-shift', 'bdv_bn_backward_split', relu_mask=None, relu_scale=ADDR['relu_scale'], relu_shift=ADDR['relu_shift'] + OFF4)
    # bdv_bn_backward_pair
    add('stat-partial-rows-0', 'bdv_bn_backward_pair', stat_partial=ADDR['stat_partial'])
    add('stat-partial-misaligned', 'bdv_bn_backward_pair', stat_partial=ADDR['stat_partial'] + OFF4, stat_rows=3)
    add('dya-is-dyb', 'bdv_bn_backward_pair', dyb=ADDR['dya'])
    add('dya-is-dout', 'bdv_bn_backward_pair', dya=ADDR['dout'])
    add('dyb-is-dout', 'bdv_bn_backward_pair', dyb=ADDR['dout'])
    # bdv_bn_eval_backward: what tests/test_frozen_bn_cpu.py leaves
    for n in ('dz', 'relu_act', 'y'):
        add(f'misaligned-{n}', 'bdv_bn_eval_backward', relu_mask=None if n == 'relu_act' else ADDR['relu_mask'], **{n: ADDR[n] + OFF4})
    add('misaligned-relu-mask', 'bdv_bn_eval_backward', relu_mask=ADDR['relu_mask'] + OFF1)
    add('dy-is-dout', 'bdv_bn_eval_backward', dy=ADDR['dout'])
    add('dz-is-dout', 'bdv_bn_eval_backward', dz=ADDR['dout'])
    for n in ('running_mean', 'invstd', 'workspace'):
        add(f'stats-null-{n}', 'bdv_bn_eval_backward', **dict(EVAL_STATS, **{n: None}))
        add(f'stats-misaligned-{n}', 'bdv_bn_eval_backward', **dict(EVAL_STATS, **{n: ADDR[n] + OFF4}))
    add('dy-is-y', 'bdv_bn_eval_backward', **dict(EVAL_STATS, dy=ADDR['y']))
    add('dz-is-y', 'bdv_bn_eval_backward', **dict(EVAL_STATS, dz=ADDR['y']))
    add('workspace-too-small', 'bdv_bn_eval_backward', **dict(EVAL_STATS, workspace_bytes=4096))
    # bdv_bn_backward_maxpool_split
    for k, v in (('N', 0), ('H', 1), ('W', 1), ('C', 16), ('C', 48), ('C', 96)):
        add(f'{k}-{v}', 'bdv_bn_backward_maxpool_split', **{k: v})
    add('misaligned-pool-idx', 'bdv_bn_backward_maxpool_split', pool_idx=ADDR['pool_idx'] + OFF1)
    add('tensor-too-large', 'bdv_bn_backward_maxpool_split', N=1 << 20, H=64, W=64)
    add('row-too-wide', 'bdv_bn_backward_maxpool_split', N=1, H=2, W=300000)
    # bdv_relu_bwd, bdv_add
    add('numel-0', 'bdv_relu_bwd', numel=0)
    add('numel-36', 'bdv_relu_bwd', numel=36)
    add('misaligned-add', 'bdv_relu_bwd', add=ADDR['add'] + OFF4)
    add('numel-0', 'bdv_add', numel=0)
    add('numel-6', 'bdv_add', numel=6)
    return out


CASES = _cases()


def refusal(entry, changed):
    """(return code, bdv_last_error()) of one call."""
    args = {n: SCALARS[n] if n in SCALARS else None if n in OPTIONAL else ADDR[n] for n in ARGS[entry]}
    args.update(BASE.get(entry, {}))
    args.update(changed)
    lib = bd._lib.lib()
    rc = getattr(lib, entry)(*[args[n] for n in ARGS[entry]])
    return rc, lib.bdv_last_error().decode()


def test_cases_cover_every_entry_point_and_the_golden():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(c[0] for c in CASES) and len({c[0] for c in CASES}) == len(CASES)
    assert {c[1] for c in CASES} == set(ARGS)
    for entry, names in ARGS.items():
        assert len(bd._lib.SIGNATURES[entry][1]) == len(names), entry
    assert {v[0] for v in want.values()} == {-1, -2}         # BDV_EINVAL and BDV_EWORKSPACE both occur


@pytest.mark.parametrize('cid,entry,changed', CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, entry, changed):
    with open(GOLDEN) as f:
        want = json.load(f)[cid]
    rc, text = refusal(entry, changed)
    assert rc != 0 and [rc, text] == want
    assert text.startswith('bdv_'), text            # refused by an argument check of the library, not by a launch


if __name__ == '__main__':
    table = {cid: list(refusal(entry, changed)) for cid, entry, changed in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + '\n}\n')
    print('wrote', len(table), 'cases')
