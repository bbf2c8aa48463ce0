"""The split-finalize and pair-backward entry points: ``include/bdvcil_hip.h``, the ctypes table in ``_lib.py`` and the built
library agree on the symbols and on how many arguments each takes; the planner and the scratch size answer without a GPU."""
import ctypes
import os
import re

import bdvcil_amd as bd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ('bdv_bn_finalize_scratch_bytes', 'bdv_bn_finalize_splits', 'bdv_bn_train_finalize_split', 'bdv_bn_backward_split',
       'bdv_bn_backward_maxpool_split', 'bdv_bn_pair_workspace_bytes', 'bdv_bn_backward_pair')
# the split form of an entry point = its arguments + (splits, fin_scratch, fin_scratch_bytes) in front of the stream
SPLIT_OF = {'bdv_bn_train_finalize_split': 'bdv_bn_train_finalize', 'bdv_bn_backward_split': 'bdv_bn_backward',
            'bdv_bn_backward_maxpool_split': 'bdv_bn_backward_maxpool'}


def _header_params(hdr, name):
    m = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\((.*?)\);', hdr, re.S | re.M)
    assert m, f'{name} is not declared in include/bdvcil_hip.h'
    return [p.strip() for p in m.group(1).split(',')]


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    for name in NEW:
        params = _header_params(hdr, name)
        assert hasattr(lib, name), f'{name} is not exported by the built library'
        assert name in bd._lib.SIGNATURES, f'{name} has no ctypes signature'
        res, args = bd._lib.SIGNATURES[name]
        assert len(args) == len(params), (name, len(args), params)
        for p, a in zip(params, args):       # pointers against pointers, scalars against scalars
            assert ('*' in p) == (a is bd._lib.P), (name, p, a)
    for new, old in SPLIT_OF.items():
        a_new, a_old = bd._lib.SIGNATURES[new][1], bd._lib.SIGNATURES[old][1]
        assert a_new == a_old[:-1] + [ctypes.c_int, bd._lib.P, ctypes.c_size_t, bd._lib.P], new
        p_new, p_old = _header_params(hdr, new), _header_params(hdr, old)
        assert [re.sub(r'\s+', ' ', p) for p in p_new[:len(p_old) - 1]] == [re.sub(r'\s+', ' ', p) for p in p_old[:-1]], new
    assert bd._lib.lib().bdv_abi_version() == bd._lib.ABI_VERSION == 33


def test_planner_and_scratch_size_answer_on_the_host():
    lib = bd._lib.lib()
    for C in (64, 128, 256, 512, 1024, 2048):
        assert lib.bdv_bn_finalize_scratch_bytes(C) >= 2 * 16 * C * 8 + C       # group sums (fp64) + C / 4 ticket words
        assert lib.bdv_bn_finalize_scratch_bytes(C) % 16 == 0
        for rows in (1, 98, 392, 1568, 2048, 6272, 8192, 25088):
            S = lib.bdv_bn_finalize_splits(rows, C)
            assert S in (1, 2, 4, 8, 16), (rows, C, S)
    assert lib.bdv_bn_finalize_splits(98, 2048) == 1            # a small slab stays on the one-block kernel
    assert lib.bdv_bn_finalize_splits(25088, 64) > 1            # the stem's does not
    assert lib.bdv_bn_pair_workspace_bytes(1, 64) > lib.bdv_bn_workspace_bytes(1, 64)


def test_split_needs_scratch():
    """An explicit split without scratch is an argument error, not a quiet run of the one-block kernel."""
    lib = bd._lib.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the call fails on its arguments before any launch
    rc = lib.bdv_bn_train_finalize_split(one, 8, 8, 64, one, one, 1e-5, 0.1, None, None, one, one, one, one, 4, None, 0, None)
    assert rc == -1 and b'scratch' in lib.bdv_last_error()
    rc = lib.bdv_bn_train_finalize_split(one, 8, 8, 64, one, one, 1e-5, 0.1, None, None, one, one, one, one, 3, None, 0, None)
    assert rc == -1 and b'splits' in lib.bdv_last_error()
