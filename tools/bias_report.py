"""Background reliance of every task checkpoint of a finished CIL run.

    python tools/bias_report.py WORK_DIR CONFIG [--det-file F] [--bg-dir D] [--tasks 0 1 ...] [--overlays N]
        [--target-layer backbone.layer4] [--conv-arith M] [--seed S] [--batch-size B] [--device D] [--threads T]

For each ``WORK_DIR/ckpt/ckpt_task_<i>.pt`` the validation sets of tasks 0..i are evaluated three ways, and ``WORK_DIR/bias_report.txt``
and ``WORK_DIR/bias_report.json`` hold, per task checkpoint:

  cnn_top1          the average CNN accuracy ``cnn_result.txt`` already lists for that task (blank without the file), for orientation
  scene_only_top1   top-1 when every clip is its video's extracted background image (``bdvcil_amd.bias.scene_only_accuracy``): the
                    backgrounds are looked up in the config's ``data.train.bg_dir`` (or ``--bg-dir``), never extracted here; videos
                    without one are counted (``scene_missing``)
  actor_attention   mean share of the Grad-CAM map inside the person boxes of ``--det-file`` (``bdvcil_amd.bias.actor_attention``);
                    only with ``--det-file``
  and the number of clips each figure rests on.

``--overlays N`` also writes the Grad-CAM overlays of the first N validation clips per task to ``WORK_DIR/bias_overlays/
task_<i>_clip_<k>.jpg`` (the clip's frames side by side, encoded by ``bdvcil_amd.encode_jpeg``).  Files are written through a
temporary name and an atomic rename."""
import argparse
import glob
import json
import os
import pathlib
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONV_ARITH_MODES = ('bf16x3', 'f32mfma', 'bf16x2', 'f16x2', 'bf16x1')        # bdvcil_amd.CONV_ARITH_MODES without 'bf16' (no eval-mode backward)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('work_dir')
    ap.add_argument('config')
    ap.add_argument('--det-file', default=None, help='human detections (.npy, the ActorCutMix file): adds the actor-attention column')
    ap.add_argument('--bg-dir', default=None, help="directory of the extracted backgrounds (default: the config's data.train.bg_dir)")
    ap.add_argument('--tasks', type=int, nargs='+', default=None, help='task checkpoints to report (default: every one found)')
    ap.add_argument('--overlays', type=int, default=0, help='write the overlays of the first N validation clips per task')
    ap.add_argument('--target-layer', default='backbone.layer4')
    ap.add_argument('--conv-arith', choices=CONV_ARITH_MODES, default=None)
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--batch-size', type=int, default=8)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--threads', type=int, default=8, help='host threads of the JPEG entropy stage')
    return ap


def find_checkpoints(work_dir, tasks=None):
    """{task index: path} of the ``ckpt/ckpt_task_<i>.pt`` files of ``work_dir``; ``tasks`` restricts (and requires) them.  A work_dir
    without any raises ``FileNotFoundError``: there is nothing to report on."""
    found = {}
    for p in glob.glob(os.path.join(str(work_dir), 'ckpt', 'ckpt_task_*.pt')):
        m = re.fullmatch(r'ckpt_task_(\d+)\.pt', os.path.basename(p))
        if m:
            found[int(m.group(1))] = p
    if not found:
        raise FileNotFoundError(f'{work_dir}: no ckpt/ckpt_task_<i>.pt -- not the work_dir of a finished run')
    if tasks is not None:
        missing = [t for t in tasks if t not in found]
        if missing:
            raise FileNotFoundError(f'{work_dir}: no checkpoint for task(s) {missing} (found {sorted(found)})')
        found = {t: found[t] for t in tasks}
    return dict(sorted(found.items()))


def cnn_result_averages(work_dir):
    """{task index: the Avg column} of ``cnn_result.txt`` (``print_mean_accuracy``'s table); empty without the file."""
    path = os.path.join(str(work_dir), 'cnn_result.txt')
    out = {}
    if os.path.exists(path):
        for line in open(path):
            m = re.match(r'\s*task (\d+)\s.*?(-?\d+\.\d+|nan)\s*$', line)
            if m:
                out[int(m.group(1))] = float(m.group(2))
    return out


def report_table(rows, with_attention):
    """The summary table of bias_report.txt, formatted as the result files' tables are (tabulate, two decimals, blanks for absent)."""
    from tabulate import tabulate
    headers = ['task', 'cnn_top1', 'scene_only_top1', 'scene_clips', 'scene_missing']
    keys = ['cnn_top1', 'scene_only_top1', 'scene_clips', 'scene_missing']
    if with_attention:
        headers += ['actor_attention', 'attention_clips', 'attention_undefined']
        keys += ['actor_attention', 'attention_clips', 'attention_undefined']
    body = [[f'task {r["task"]}'] + [r.get(k) for k in keys] for r in rows]
    return tabulate(body, headers=headers, floatfmt=['.2f', '.2f', '.2f', 'd', 'd', '.4f', 'd', 'd'][:len(headers)], missingval='')


def json_ready(x):
    """NaN (an undefined mean) becomes null: the file stays standard JSON."""
    if isinstance(x, float) and x != x:
        return None
    if isinstance(x, dict):
        return {k: json_ready(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_ready(v) for v in x]
    return x


def write_atomic(path, data: bytes):
    from bdvcil_amd.background import _write_atomic
    _write_atomic(pathlib.Path(path), data)


def main(argv=None):
    args = build_parser().parse_args(argv)
    ckpts = find_checkpoints(args.work_dir, args.tasks)                 # before anything touches the GPU

    import bdvcil_amd as bd
    import numpy as np
    import torch
    from bdvcil_amd import bias
    from bdvcil_amd.task_loop import print_mean_accuracy
    if args.seed is not None:
        import random
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    cfg = bd.load_config(args.config)
    arith = args.conv_arith or cfg.get('conv_arith')
    if arith == 'bf16':
        raise SystemExit("bias_report: conv_arith 'bf16' stores activations in bf16, which has no eval-mode backward; use bf16x1")
    spec = bd.clip_loader_spec(cfg)
    loader = bd.build_clip_loader(cfg, device=device, seed=args.seed, threads=args.threads)
    kw = spec['kwargs']
    bg_dir = args.bg_dir or spec['dataset'].get('bg_dir')
    if not bg_dir:
        raise SystemExit('bias_report: the config names no data.train.bg_dir; pass --bg-dir')
    splits = bd.TaskSplits(cfg.task_splits)
    files = bd.CILWorkDir(args.work_dir, splits, cfg.get('cil_ann_file_template', '{}_task_{}.txt'))
    files.collect_ann_files_from_work_dir(len(splits.task_splits))
    val = [bd.RawframeRecords(str(p), cfg.data_root, test_mode=True, phase='val') for p in files.task_splits_ann_files['val'][:max(ckpts) + 1]]
    model = bd.build_model(cfg.model).to(device)
    cnn_avg = cnn_result_averages(args.work_dir)
    decoder = bd.JpegDecoder(device, args.threads)
    overlay_dir = pathlib.Path(args.work_dir) / 'bias_overlays'
    rows, meters = [], []

    import contextlib
    with (bd.conv_arith(arith) if arith else contextlib.nullcontext()):
        for t, path in ckpts.items():
            model.update_fc(splits.num_classes(t))
            model.load_state_dict(torch.load(path, map_location=device, weights_only=True))
            model.eval()
            records = bd.RawframeRecords(None, None, test_mode=True, phase='val').extend(val[:t + 1])
            sizes = [len(v) for v in val[:t + 1]]
            bg_files = bd.resolve_bg_files(records.video_infos, bg_dir, extract_bg_if_not_found=False,
                                           bg_image_extension=spec['dataset'].get('bg_image_extension', '.jpg'))
            scene = bias.scene_only_accuracy(model, records, bg_files, task_sizes=sizes, num_segments=kw['num_segments'],
                                             short_edge=kw['short_edge'], input_size=kw['input_size'], batch_size=args.batch_size,
                                             decoder=decoder)
            meters.append(scene['meter'])
            row = {'task': t, 'checkpoint': os.path.relpath(path, args.work_dir), 'cnn_top1': cnn_avg.get(t),
                   'scene_only_top1': scene['overall'], 'scene_only_per_task': scene['per_task'], 'scene_clips': scene['clips'],
                   'scene_missing': scene['missing'], 'scene_missing_videos': scene['missing_videos']}
            cam = bd.GradCAM(model, args.target_layer)
            if args.det_file:
                att = bias.actor_attention(model, loader, records, args.det_file, batch_size=args.batch_size, cam=cam)
                row.update(actor_attention=att['mean'], actor_attention_per_class={str(c): v for c, v in att['per_class'].items()},
                           attention_clips=att['clips'], attention_undefined=att['undefined'])
            if args.overlays > 0:
                infos = records.video_infos[:args.overlays]
                batch = loader(infos, 'val')
                ov = cam(batch['imgs'], batch['label'], overlay=True)['overlay']
                overlay_dir.mkdir(parents=True, exist_ok=True)
                names = []
                for k, data in enumerate(bd.encode_jpeg([bias.overlay_strip(ov[k]) for k in range(len(infos))], device=device)):
                    write_atomic(overlay_dir / f'task_{t}_clip_{k}.jpg', data)
                    names.append(f'bias_overlays/task_{t}_clip_{k}.jpg')
                row['overlays'] = names
            rows.append(row)

    task_sizes = [len(c) for c in splits.task_splits]
    text = 'Bias report (target layer {}, conv arithmetic {})\n'.format(args.target_layer, arith or bd.get_conv_arith())
    text += report_table(rows, bool(args.det_file)) + '\n'
    if list(ckpts) == list(range(len(ckpts))):          # the result files' layout needs task 0..n without gaps
        text += '\nScene-only accuracies' + print_mean_accuracy(meters, task_sizes[:len(meters)]) + '\n'
    report = {'work_dir': os.path.abspath(args.work_dir), 'target_layer': args.target_layer, 'conv_arith': arith or bd.get_conv_arith(),
              'det_file': args.det_file, 'bg_dir': str(bg_dir), 'tasks': rows}
    write_atomic(os.path.join(args.work_dir, 'bias_report.txt'), text.encode())
    write_atomic(os.path.join(args.work_dir, 'bias_report.json'), (json.dumps(json_ready(report), indent=1) + '\n').encode())
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
