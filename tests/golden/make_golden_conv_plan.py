"""Writes tests/golden/conv_plan_sites.json: what ``kernels.conv_plan`` answers (kernel, reads_planes, stat_rows, splits, pre_ok, or
0 where the library refuses) for every conv geometry of the models and the conv tests, in every arithmetic.  Host-only: no GPU is
touched.

    python tests/golden/make_golden_conv_plan.py [out.json]

The table pins the dispatch: a change of the planner that moves a site to another kernel or resizes a side buffer shows up as a
diff of this file.  One geometry per line, its plans in the order of ``params``; kernel names are stored once ("kernels") and
referenced by index.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from bdvcil_amd import kernels as K                     # noqa: E402
from bdvcil_amd._lib import check, lib                  # noqa: E402

FRAMES = (8, 64, 256)
KINDS = ('fprop', 'dgrad', 'wgrad')
# (name, set_conv_arith mode, act_dtype of the geometry)
ARITHS = (('f32mfma', 'f32mfma', 0), ('bf16x3', 'bf16x3', 0), ('bf16x2', 'bf16x2', 0), ('bf16x1', 'bf16x1', 0), ('bf16', 'bf16', 1))
T = 8


def _sites():
    """(label, geometry factory of the frame count)."""
    from test_conv_gpu import CASES
    from test_conv_sites_gpu import SITES
    out = []
    for Cin, Cout, k, st, H, shift in SITES:            # TSM-R50
        c = 4 if Cin == 3 else Cin
        out.append((f'r50 {Cin}->{Cout} k{k} s{st} @{H} shift{shift}',
                    lambda N, a=(H, H, c, Cout, k, k, st, k // 2, T if shift else 1, c // 8 if shift else 0): K.make_geom(N, *a)))
    for i, (C, H) in enumerate(((64, 56), (128, 28), (256, 14), (512, 7))):      # BasicBlock (R18 / R34)
        for shift in (0, 1):
            out.append((f'basic {C}->{C} k3 s1 @{H} shift{shift}',
                        lambda N, a=(H, H, C, C, 3, 3, 1, 1, T if shift else 1, C // 8 if shift else 0): K.make_geom(N, *a)))
            if i:
                out.append((f'basic {C // 2}->{C} k3 s2 @{2 * H} shift{shift}',
                            lambda N, a=(2 * H, 2 * H, C // 2, C, 3, 3, 2, 1, T if shift else 1, C // 16 if shift else 0): K.make_geom(N, *a)))
        if i:
            out.append((f'basic {C // 2}->{C} k1 s2 @{2 * H} downsample', lambda N, a=(2 * H, 2 * H, C // 2, C, 1, 1, 2, 0): K.make_geom(N, *a)))
    # I3D: the inflated 3x1x1 conv1 of each stage's first and later blocks (clips of 8 frames), the fused 5x7x7 stem
    for Cin, Cout, H in ((64, 64, 56), (256, 64, 56), (256, 128, 56), (512, 128, 28), (512, 256, 28), (1024, 256, 14), (1024, 512, 14),
                         (2048, 512, 7)):
        out.append((f'i3d {Cin}->{Cout} kt3 @{H}', lambda N, a=(T, H, H, Cin, Cout, 3): K.make_temporal_geom(N // T, *a)))
    out.append(('i3d stem 5x7x7 @224', lambda N: K.make_geom(N, 224, 224, 4, 64, 7, 7, 2, 3, T=T, rt=5, st_t=2)))
    for _, H, W, Cin, Cout, R, st, pad, Tc, fold in CASES:                        # tests/test_conv_gpu.py
        out.append((f'case {H}x{W} {Cin}->{Cout} k{R} s{st} p{pad} T{Tc} fold{fold}',
                    lambda N, a=(H, W, Cin, Cout, R, R, st, pad, Tc, fold): K.make_geom(N, *a)))
    return out


def params(N):
    """(kind, arith, pre, forced tile) of every plan taken per geometry, in the order of a geometry's results."""
    out = []
    for arith, _, _ in ARITHS:
        for tile in ((-1,) + tuple(range(7)) if arith == 'bf16x3' and N == 64 else (-1,)):
            for kind in KINDS:
                out += [(kind, arith, pre, tile) for pre in ((0, 1) if arith == 'bf16x3' and kind != 'dgrad' else (0,))]
    return out


def build_table():
    names, geoms = [], []

    def plan(g, kind, pre):
        try:
            p = K.conv_plan(g, kind, pre=bool(pre))
        except (ValueError, RuntimeError):
            return 0
        name = p.kernel.decode()
        if name not in names:
            names.append(name)
        return [names.index(name), p.reads_planes, p.stat_rows, p.splits, p.pre_ok]

    modes = {arith: (mode, act) for arith, mode, act in ARITHS}
    try:
        for label, make in _sites():
            for N in FRAMES:
                g = make(N)
                res = []
                for kind, arith, pre, tile in params(N):
                    K.set_conv_arith(modes[arith][0])
                    g.act_dtype = modes[arith][1]
                    check(lib().bdv_conv_debug_force_tile(tile), 'bdv_conv_debug_force_tile')
                    res.append(plan(g, kind, pre))
                geoms.append([label, N, res])
    finally:
        check(lib().bdv_conv_debug_force_tile(-1), 'bdv_conv_debug_force_tile')
        K.set_conv_arith('bf16x3')
    return {'result': ['kernel', 'reads_planes', 'stat_rows', 'splits', 'pre_ok', '(0 = refused)'],
            'params': [list(q) for q in params(8)], 'params_n64': [list(q) for q in params(64)], 'kernels': names, 'geoms': geoms}


def dumps(table):
    """One geometry per line, its results in the order of "params" ("params_n64" at 64 frames)."""
    def block(key, sep):
        return ' "%s": [\n%s\n ]' % (key, ',\n'.join(json.dumps(v, separators=sep) for v in table[key]))
    head = ',\n'.join(' "%s": %s' % (k, json.dumps(table[k], separators=(',', ':'))) for k in ('result', 'params', 'params_n64'))
    return '{\n%s,\n%s,\n%s\n}\n' % (head, block('kernels', (', ', ': ')), block('geoms', (',', ':')))


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_plan_sites.json')
    with open(out, 'w') as f:
        f.write(dumps(build_table()))
    print('wrote', out)
