"""Dump the settings ``bdvcil_amd.config_run.clip_loader_spec`` reads from the reference's CIL configs, one config per dataset family.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cil_configs.py

Each config file is imported by path with ``VIDEO_CIL_ROOT`` set to a placeholder.  Written to ``tests/golden/cil_configs.json``, per
config: ``data.train`` / ``val`` / ``test`` / ``features_extraction`` (the four pipelines inside them) without ``ann_file``,
``features_extraction_epochs``, and ``methods``, ``randAug_prob``, ``videos_per_gpu``, ``accumulate_grad_batches``.  Settings only."""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cil_configs.json')
CONFIGS = [
    'ucf101/bgmix_plus_randAug/bgmix_seed_1000_inc_10_stages_bgmix_plus_randAug.py',
    'ucf101/bgmix_only/seed_1000_inc_5_stages_bgmix_only.py',
    'ucf101/randaug_only/seed_1000_inc_5_stages_randAug_only.py',
    'ucf101/no_aug/seed_1000_inc_10_stages_no_aug.py',
    'ucf101/icarl/icarl_seed_1000_inc_10_stages_bgmix_plus_randAug.py',
    'ucf101/icarl_video_mix/icarl_seed_1000_inc_10_stages_video_mix.py',
    'ucf101/seed_1000_inc_10_stages_ActorCutMix_plus_randAug.py',
    'ucf101/predefined_background/seed_1000_inc_10_stages_bgmix_plus_randAug_place365_bg.py',
    'sth-sthv2/seed_1000_inc_18_stages_bgmix_plus_randAug.py',
    'HMDB51/bgmix_seed_1000_inc_5_stages_bgmix_plus_randAug.py',
]


def main():
    os.environ['VIDEO_CIL_ROOT'] = 'VIDEO_CIL_ROOT'
    out = {}
    for k, rel in enumerate(CONFIGS):
        spec = importlib.util.spec_from_file_location(f'ref_cfg_{k}', os.path.join(REF, 'configs', rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        data = {}
        for part in ('train', 'val', 'test', 'features_extraction'):
            data[part] = {key: v for key, v in mod.data[part].items() if key != 'ann_file'}
        data['features_extraction_epochs'] = mod.data.get('features_extraction_epochs', 1)
        out[rel] = dict(data=data, methods=mod.methods, randAug_prob=getattr(mod, 'randAug_prob', None),
                        videos_per_gpu=mod.videos_per_gpu, accumulate_grad_batches=getattr(mod, 'accumulate_grad_batches', 1))
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
