"""The conv dispatch, pinned on the host: ``kernels.conv_plan`` (one ``bdv_conv_plan_query`` per call) must answer what
tests/golden/conv_plan_sites.json recorded for every conv site of the models and the conv tests, in every arithmetic, with and
without the producer's BatchNorm in the loader and under every forced tile: kernel, reads_planes, stat_rows, splits, pre_ok, or a
refusal.  The table was recorded from the selection logic as it stood before the planner (spread over the Python wrappers, the
``_pl`` entry points, the name and the sizing queries); tests/golden/make_golden_conv_plan.py regenerates it.  No GPU needed."""
import ctypes
import importlib.util
import json
import os

import bdvcil_amd as bd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_golden_conv_plan', os.path.join(GOLDEN, 'make_golden_conv_plan.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_table_is_unchanged():
    gen = _generator()
    table = gen.build_table()
    with open(os.path.join(GOLDEN, 'conv_plan_sites.json')) as f:
        text = f.read()
    want = json.loads(text)
    assert table['kernels'] == want['kernels'] and len(table['geoms']) == len(want['geoms'])
    for (label, N, got), (wlabel, wN, exp) in zip(table['geoms'], want['geoms']):
        assert (label, N, len(got)) == (wlabel, wN, len(exp))
        for q, g, e in zip(gen.params(N), got, exp):
            assert g == e, f'{label} at {N} frames, {q}: {g} != {e}'
    assert gen.dumps(table) == text                     # regenerating the file changes no byte


def test_no_plan_names_a_retired_kernel():
    """The kernels this table was recorded to retire: the weight gradient that split both operands in the K loop, and the
    fprop / dgrad instantiations that split the weights there (``..., false>``)."""
    gen = _generator()
    with open(os.path.join(GOLDEN, 'conv_plan_sites.json')) as f:
        want = json.load(f)
    names = want['kernels']
    assert any(n.startswith('conv_fprop_x3_kernel') for n in names) and any(n.startswith('conv_dgrad_x3_kernel') for n in names)
    for n in names:
        assert not n.startswith('conv_wgrad_x3_kernel'), n
        assert not ('_x3_kernel' in n and n.replace(' ', '').endswith(',false>')), n
    plans = [(q[0], r) for _, N, res in want['geoms'] for q, r in zip(gen.params(N), res)]
    assert len(plans) == sum(len(res) for _, _, res in want['geoms'])
    assert {r[0] for _, r in plans if r != 0} == set(range(len(names)))
    # every kind has refusals and plans, and the plans carry the buffer sizes of their kind
    for kind, col in (('fprop', 2), ('dgrad', 2), ('wgrad', 3)):
        rows = [r for k, r in plans if k == kind]
        assert any(r == 0 for r in rows)
        assert all(r[col] > 0 for r in rows if r != 0)


def test_retired_entry_points_are_gone():
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    for name in ('fprop_stat_rows', 'fprop_pl_stat_rows', 'fprop_pre_stat_rows', 'dgrad_stat_rows', 'dgrad_pl_stat_rows', 'wgrad_splits',
                 'wgrad_pl_splits', 'uses_planes', 'kernel_name', 'fprop_pre_ok', 'wgrad_pre_ok', 'fprop_x3', 'dgrad_x3', 'wgrad_partial_x3'):
        assert not hasattr(lib, 'bdv_conv_' + name), name
        assert 'bdv_conv_' + name not in bd._lib.SIGNATURES
