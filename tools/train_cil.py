"""Run a CIL config file end to end: train every task of the config, or re-test the checkpoints of a finished run.

    VIDEO_CIL_ROOT=/data/ucf101 python tools/train_cil.py CONFIG [--test] [--test-nme] [--prefetch N] [--seed S] [--device D]
        [--conv-arith {bf16x3,f32mfma,bf16x2,f16x2,bf16x1,bf16}] [--kd-type {mse,pod,pod_spatial,pod_flat}]
        [--fg-merge-prob P [--fg-merge-beta B]] [--kd-importance [--kd-importance-mix X]]

CONFIG is a config file of the reference (configs/ucf101/..., self-contained Python that reads VIDEO_CIL_ROOT).  The clip loader is
built from the config's ``data.train`` and its four pipelines (``bdvcil_amd.clip_loader_spec``; a stage the loaders cannot honour is an
error, not a guess), and ``CILTaskLoop`` leaves the reference's files in the config's ``work_dir``; training ends with the re-test of
every task's checkpoint (``cnn_result.txt``; with ``--test-nme`` also ``nme_result.txt``), and ``--test`` does only that.  ``--seed`` seeds the loader's own generators,
the shuffle and the process-global generators the training step draws from, which makes a run reproducible at any ``--prefetch``.
``--conv-arith`` sets the config's ``conv_arith`` key (the conv arithmetic of everything the loop computes; it wins over the config
file, and without either the default arithmetic runs); the files of the work_dir are fp32 in every mode, so a run trained under one
mode re-tests under any other.
``--kd-type`` sets the config's ``kd_type`` key: the feature-distillation loss of ``methods='base'``, the reference's MSE or PODNet's
pooled-output losses ('pod' = POD-spatial on feature maps, POD-flat on pooled features); it wins over the config file.
``--fg-merge-prob P`` sets the config's ``fg_merge`` key: foreground merging of the training batches (a clip keeps its motion
foreground and takes the rest from another clip of the batch, with probability P; labels untouched), ``--fg-merge-beta B`` the share
of pixels kept as foreground (default 0.5); both win over the config file, whose other ``fg_merge`` entries stay.
``--kd-importance`` sets the config's ``kd_importance`` key to ``dict(type='time_channel')``: after every task the loop estimates a
time-channel importance map per 'mse' distillation module and weights the next task's MSE with it; ``--kd-importance-mix X`` (in
[0, 1], default 0) mixes the map toward uniform.  Both win over the config file, whose other ``kd_importance`` entries stay.
Several GPUs: start one process per GPU with torchrun; the process group is picked up from the environment."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


KD_TYPES = ('mse', 'pod', 'pod_spatial', 'pod_flat')                               # bdvcil_amd.KD_TYPES (checked in main)
CONV_ARITH_MODES = ('bf16x3', 'f32mfma', 'bf16x2', 'f16x2', 'bf16x1', 'bf16')      # bdvcil_amd.CONV_ARITH_MODES (checked in main)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('config')
    ap.add_argument('--test', action='store_true', help='re-test the checkpoints of the work_dir instead of training')
    ap.add_argument('--test-nme', action='store_true', help='test the nearest-mean-of-exemplars classifier too')
    ap.add_argument('--prefetch', type=int, default=2, help='batches loaded ahead on a worker thread (0 = inline)')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--device', default=None)
    ap.add_argument('--threads', type=int, default=8, help='host threads of the JPEG entropy stage')
    ap.add_argument('--conv-arith', choices=CONV_ARITH_MODES, default=None,
                    help="conv arithmetic of the run (the config's conv_arith key; default: the config's, else bf16x3)")
    ap.add_argument('--kd-type', choices=KD_TYPES, default=None,
                    help="feature-distillation loss of methods='base' (the config's kd_type key; default: the config's, else mse)")
    ap.add_argument('--fg-merge-prob', type=float, default=None,
                    help="foreground merging of the training batches with this probability per clip (the config's fg_merge key)")
    ap.add_argument('--fg-merge-beta', type=float, default=None,
                    help='share of the pixels kept as foreground (with --fg-merge-prob or an fg_merge key of the config; default 0.5)')
    ap.add_argument('--kd-importance', action='store_true',
                    help="time-channel importance weighting of the 'mse' distillation (the config's kd_importance key)")
    ap.add_argument('--kd-importance-mix', type=float, default=None,
                    help='mix the importance map toward uniform by this share (with --kd-importance or a kd_importance key of the config)')
    return ap


def set_kd_importance(cfg, on=False, mix=None):
    """--kd-importance / --kd-importance-mix -> the config's ``kd_importance`` key; entries of the config file that no flag names stay."""
    if not on and mix is None:
        return cfg
    if not on and not cfg.get('kd_importance'):
        raise SystemExit('--kd-importance-mix needs --kd-importance (the config has no kd_importance key)')
    spec = dict(cfg.get('kd_importance') or {})
    spec.setdefault('type', 'time_channel')
    if mix is not None:
        spec['mix'] = mix
    cfg['kd_importance'] = spec
    return cfg


def set_fg_merge(cfg, prob=None, beta=None):
    """--fg-merge-prob / --fg-merge-beta -> the config's ``fg_merge`` key; entries of the config file that no flag names stay."""
    if prob is None and beta is None:
        return cfg
    if prob is None and not cfg.get('fg_merge'):
        raise SystemExit('--fg-merge-beta needs --fg-merge-prob (the config has no fg_merge key)')
    spec = dict(cfg.get('fg_merge') or {})
    if prob is not None:
        spec['prob'] = prob
    if beta is not None:
        spec['beta'] = beta
    cfg['fg_merge'] = spec
    return cfg


def main(argv=None):
    args = build_parser().parse_args(argv)

    import bdvcil_amd as bd           # before the first torch.cuda call (GPU_MAX_HW_QUEUES)
    assert tuple(bd.CONV_ARITH_MODES) == CONV_ARITH_MODES and tuple(bd.KD_TYPES) == KD_TYPES
    import torch
    import torch.distributed as dist
    local = int(os.environ.get('LOCAL_RANK', 0))
    device = args.device or f'cuda:{local}'
    torch.cuda.set_device(torch.device(device))
    if int(os.environ.get('WORLD_SIZE', 1)) > 1 and not dist.is_initialized():
        dist.init_process_group('nccl')
    if args.seed is not None:
        import random
        import numpy as np
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    cfg = bd.load_config(args.config)
    if args.conv_arith is not None:
        cfg['conv_arith'] = args.conv_arith
    if args.kd_type is not None:
        cfg['kd_type'] = args.kd_type
    set_fg_merge(cfg, args.fg_merge_prob, args.fg_merge_beta)
    bd.task_loop.check_loop_fg_merge(cfg)
    set_kd_importance(cfg, args.kd_importance, args.kd_importance_mix)
    bd.task_loop.check_loop_kd_importance(cfg)
    rank = dist.get_rank() if dist.is_initialized() else 0
    # each rank loads its own share of an epoch: its loader draws from its own stream
    loader = bd.build_clip_loader(cfg, device=device, seed=None if args.seed is None else args.seed + rank, threads=args.threads)

    def make_loop():
        return bd.CILTaskLoop(cfg, loader, device=device, seed=args.seed or 0, prefetch=args.prefetch)

    try:
        if not args.test:
            loop = make_loop()
            try:
                loop.train()
            finally:
                loop.close()
        # the accuracy tables of every task's checkpoint: the last thing a training run does, and all that --test does
        loop = make_loop()
        try:
            tables = loop.cil_testing(test_nme=args.test_nme)
        finally:
            loop.close()
        if rank == 0:
            for name in sorted(tables):
                print(tables[name])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
