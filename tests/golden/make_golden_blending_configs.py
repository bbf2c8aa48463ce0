"""Dump the ``model`` dicts of the reference's two ``train_cfg.blending`` configs (Mixup and CutMix on TSM-R50, sth-sth v1).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_blending_configs.py

Each config file is imported by path (its ``_base_`` list is a plain module attribute and is not followed: the ``model`` dict is written
out in full in both files).  Written to ``tests/golden/blending_configs.json``, per config: ``model``.  Settings only."""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'blending_configs.json')
CONFIGS = [
    'recognition/tsm/tsm_r50_mixup_1x1x8_50e_sthv1_rgb.py',
    'recognition/tsm/tsm_r50_cutmix_1x1x8_50e_sthv1_rgb.py',
]


def main():
    out = {}
    for k, rel in enumerate(CONFIGS):
        spec = importlib.util.spec_from_file_location(f'ref_blend_cfg_{k}', os.path.join(REF, 'configs', rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out[rel] = dict(model=mod.model)
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
