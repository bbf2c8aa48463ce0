"""tools/bias_report.py on a toy work_dir: 2 tasks x 2 classes of 8-frame 32 x 40 JPEG videos, backgrounds extracted by
``resolve_bg_files``, a synthetic detection file and two checkpoints of an untrained TSM-R18.  The tool runs as a fresh child process;
its json must equal direct calls of ``bias.scene_only_accuracy`` / ``bias.actor_attention`` on the same files."""
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'bias_report.py')

CONFIG = '''
task_splits = [[0, 1], [2, 3]]
data_root = {root!r}
cil_ann_file_template = '{{}}_task_{{}}.txt'
norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_bgr=False)
def _eval(crop):
    return [dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8, test_mode=True), dict(type='RawFrameDecode'),
            dict(type='Resize', scale=(-1, 64)), crop, dict(type='Normalize', **norm), dict(type='FormatShape', input_format='NCHW')]
train_pipeline = [dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8), dict(type='RawFrameDecode'),
                  dict(type='Resize', scale=(-1, 64)), dict(type='RandAugment', n=2, m=10, prob=0.75),
                  dict(type='MultiScaleCrop', input_size=64, scales=(1, 0.875), num_fixed_crops=13),
                  dict(type='Resize', scale=(64, 64), keep_ratio=False), dict(type='Normalize', **norm)]
data = dict(train=dict(type='BackgroundMixDataset', ann_file='', data_prefix=data_root, pipeline=train_pipeline, bg_dir={bg!r},
                       with_randAug=True, bg_crop_size=(64, 64), bg_resize=64),
            val=dict(type='RawframeDataset', pipeline=_eval(dict(type='CenterCrop', crop_size=64))),
            test=dict(type='RawframeDataset', pipeline=_eval(dict(type='ThreeCrop', crop_size=64))),
            features_extraction=dict(type='RawframeDataset', pipeline=_eval(dict(type='CenterCrop', crop_size=64))))
model = {model!r}
'''


def _same(a, b):
    """A value read back from the json against the direct call's: equal, an undefined mean (nan) being written as null."""
    if isinstance(b, float) and math.isnan(b):
        return a is None
    return a == b


def _pillow_jpeg(img, q=95):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'JPEG', quality=q)
    return b.getvalue()


def test_bias_report_tool(tmp_path, dev):
    import bdvcil_amd as bd
    from bdvcil_amd import bias
    from bdvcil_amd.task_loop import AverageMeter, print_mean_accuracy
    from oracle import tsm_oracle as O
    root, bg_dir, work = tmp_path / 'rawframes', tmp_path / 'bg', tmp_path / 'work'
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:32, 0:40]
    lines = {'train': [], 'val': []}
    dets = {}
    for c in range(4):
        for name, n in (('train', 1), ('val', 2)):
            for k in range(n):
                rel = f'class{c}/{name}_v{c}_{k}'
                d = root / rel
                d.mkdir(parents=True)
                base = np.stack([128 + 90 * np.sin((c + 1) * xx / 5.0), 128 + 90 * np.cos((c % 2 + 1) * yy / 4.0), np.full(xx.shape, 60.0 * c)], -1)
                for i in range(1, 9):
                    frame = base.copy()
                    frame[8:24, 4 + 3 * i:12 + 3 * i] = 255 - 40 * c          # the "actor": a bright block that moves
                    Image.fromarray(np.clip(frame + rng.normal(0, 6, frame.shape), 0, 255).astype(np.uint8)).save(
                        str(d / f'img_{i:05}.jpg'), quality=85, subsampling=2)
                lines[name].append(f'{rel} 8 {c}\n')
                # detections are read by frame number (1-based): entry 0 is never used.  One confident box on the actor, one below the
                # threshold; the second val video of class 1 has no confident box in any frame (its attention is undefined)
                score = 0.2 if (c, name, k) == (1, 'val', 1) else 0.9
                dets[f'{name}_v{c}_{k}'] = [np.array([[4.0 + 3 * i, 8.0, 12.0 + 3 * i, 24.0, score], [0.0, 0.0, 40.0, 32.0, 0.3]]) for i in range(9)]
    for name in ('train', 'val'):
        (tmp_path / f'{name}.txt').write_text(''.join(lines[name]))
    det_file = tmp_path / 'detections.npy'
    np.save(str(det_file), dets, allow_pickle=True)
    splits = bd.TaskSplits([[0, 1], [2, 3]])
    files = bd.CILWorkDir(work, splits)
    files.generate_annotation_file(str(tmp_path / 'train.txt'), str(tmp_path / 'val.txt'))
    val = [bd.RawframeRecords(str(p), str(root), test_mode=True, phase='val') for p in files.task_splits_ann_files['val']]
    assert [len(v) for v in val] == [4, 4]
    all_val = [v for r in val for v in r.video_infos]
    assert len(bd.resolve_bg_files(all_val, bg_dir)) == 8                          # extracted on the GPU, one per video
    os.unlink(bias.bg_file_for(val[1].video_infos[0]['frame_dir'], bg_dir))        # a video without a background: counted, not skipped
    model_cfg = O.r50_cfg(num_classes=2, depth=18, head='LocalSimilarityClassifier', loss='LSCLoss', dropout_ratio=0.0)
    torch.manual_seed(11)
    model = bd.build_model(model_cfg).cuda()
    torch.save(model.state_dict(), files.ckpt_file(0))
    model.update_fc(4)
    torch.save(model.state_dict(), files.ckpt_file(1))
    meters = [AverageMeter(), AverageMeter()]
    meters[0].update(75.0, 4)
    meters[1].update(50.0, 4)
    meters[1].update(25.0, 4)
    (work / 'cnn_result.txt').write_text('CNN Accuracies' + print_mean_accuracy(meters, [2, 2]) + '\n')
    cfg_path = tmp_path / 'toy_config.py'
    cfg_path.write_text(CONFIG.format(root=str(root), bg=str(bg_dir), model=model_cfg))

    run = subprocess.run([sys.executable, TOOL, str(work), str(cfg_path), '--det-file', str(det_file), '--overlays', '2', '--seed', '3',
                          '--batch-size', '4'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    text = (work / 'bias_report.txt').read_text()
    report = json.loads((work / 'bias_report.json').read_text())
    assert 'task 0' in text and 'task 1' in text and 'scene_only_top1' in text and 'actor_attention' in text and 'Scene-only accuracies' in text
    assert [r['task'] for r in report['tasks']] == [0, 1] and report['target_layer'] == 'backbone.layer4'
    assert not [p for p in work.iterdir() if p.name.endswith('.tmp')]

    cfg = bd.load_config(str(cfg_path))
    loader = bd.build_clip_loader(cfg, device='cuda', seed=3)
    direct = bd.build_model(cfg.model).cuda()
    for t, row in enumerate(report['tasks']):
        direct.update_fc(splits.num_classes(t))
        direct.load_state_dict(torch.load(files.ckpt_file(t), map_location='cuda', weights_only=True))
        direct.eval()
        records = bd.RawframeRecords(None, None, test_mode=True, phase='val').extend(val[:t + 1])
        bgs = bd.resolve_bg_files(records.video_infos, bg_dir, extract_bg_if_not_found=False)
        scene = bias.scene_only_accuracy(direct, records, bgs, task_sizes=[4] * (t + 1), short_edge=64, input_size=64, batch_size=4)
        assert row['cnn_top1'] == [75.0, 37.5][t]
        assert row['scene_only_top1'] == scene['overall'] and row['scene_only_per_task'] == scene['per_task']
        assert row['scene_clips'] == scene['clips'] == [4, 7][t] and row['scene_missing'] == scene['missing'] == [0, 1][t]
        assert row['scene_missing_videos'] == scene['missing_videos'] == ([] if t == 0 else [val[1].video_infos[0]['frame_dir']])
        assert 0.0 <= scene['overall'] <= 100.0
        att = bias.actor_attention(direct, loader, records, str(det_file), batch_size=4)
        # the same kernels on the same files in another process: nothing on the way has a float atomic, so the same bits
        assert _same(row['actor_attention'], att['mean']) and 0.0 < att['mean'] < 1.0
        assert row['attention_clips'] == att['clips'] == [3, 7][t] and row['attention_undefined'] == att['undefined'] == 1
        assert math.isnan(att['values'][3]) and set(row['actor_attention_per_class']) == {str(c) for c in att['per_class']}
        for c, v in att['per_class'].items():
            assert _same(row['actor_attention_per_class'][str(c)], v)
        # the overlays: each file decodes, through the project's own decoder, to exactly the pixels libjpeg-turbo makes of the strip
        # encode_jpeg was given (Pillow's encoder at cv2.imwrite's quality 95, then Pillow's decoder): an independent round trip, no
        # tolerance.  The distance of those pixels to the strip itself is the codec's loss and is printed only.
        batch = loader(records.video_infos[:2], 'val')
        ov = bd.GradCAM(direct)(batch['imgs'], batch['label'], overlay=True)['overlay']
        assert row['overlays'] == [f'bias_overlays/task_{t}_clip_{k}.jpg' for k in range(2)]
        for k, rel in enumerate(row['overlays']):
            strip = bias.overlay_strip(ov[k]).cpu().numpy()
            assert strip.shape == (64, 8 * 64, 3) and strip.dtype == np.uint8
            data = (work / rel).read_bytes()
            decoded = bd.JpegDecoder('cuda').decode([data])[0].cpu().numpy()
            want = np.asarray(Image.open(io.BytesIO(_pillow_jpeg(strip, 95))).convert('RGB'))
            assert np.array_equal(decoded, want)
            err = np.abs(decoded.astype(np.int32) - strip.astype(np.int32))
            print(f'task {t} overlay {k}: JPEG round trip mean |err| {err.mean():.2f}, max {err.max()} (quality 95, 4:2:0)')
    # scene_only_accuracy leaves a mixed pattern of training flags as it found it
    direct.train()
    direct.backbone.layer2.eval()
    flags = {n: m.training for n, m in direct.named_modules()}
    assert len(set(flags.values())) == 2
    bias.scene_only_accuracy(direct, val[0], bgs, short_edge=64, input_size=64, batch_size=4)
    assert {n: m.training for n, m in direct.named_modules()} == flags
    direct.eval()
    # a video missing from the detection file: KeyError, as the ActorCutMix loader raises
    del dets['val_v0_1']
    short = tmp_path / 'detections_short.npy'
    np.save(str(short), dets, allow_pickle=True)
    with pytest.raises(KeyError, match='val_v0_1'):
        bias.actor_attention(direct, loader, val[0], str(short))


def test_scene_clips_are_the_val_chain_of_a_still_video(tmp_path, dev):
    """``bias.scene_clips`` against the evaluation loader itself: a video whose eight frames are all one background image must give,
    through ``RawFrameClipLoader``'s ``val`` phase (decode -> Resize(-1, S) -> CenterCrop -> Normalize), the clip ``scene_clips`` makes
    of that image -- and against a torch CPU restatement of the crop and Normalize on the loader-independent resize."""
    import bdvcil_amd as bd
    from bdvcil_amd import bias
    from bdvcil_amd.decode import RawFrameClipLoader, rescale_size
    rng = np.random.default_rng(8)
    streams, infos = [], []
    for k, (h, w) in enumerate(((32, 40), (48, 36))):                    # landscape and portrait: both crop offsets matter
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.clip(np.stack([128 + 100 * np.sin(xx / 3.0 + k), 128 + 100 * np.cos(yy / 2.5), 8.0 * xx + 3.0 * yy], -1)
                      + rng.normal(0, 5, (h, w, 3)), 0, 255).astype(np.uint8)
        data = _pillow_jpeg(img, 90)
        d = tmp_path / f'still_{k}'
        d.mkdir()
        for i in range(1, 9):
            (d / f'img_{i:05}.jpg').write_bytes(data)
        streams.append(data)
        infos.append(dict(frame_dir=str(d), total_frames=8, label=0))
    loader = RawFrameClipLoader('cuda', short_edge=24, input_size=20, test_crop=('ThreeCrop', 24), threads=2)
    got = bias.scene_clips(streams, loader.decoder, 8, short_edge=24, input_size=20)
    assert tuple(got.shape) == (2, 8, 3, 20, 20)
    for k in range(2):
        want = loader([infos[k]], 'val')['imgs']
        assert torch.equal(got[k:k + 1], want), k
        # crop + Normalize restated on the CPU, from the resized frame (the resize kernel has its own tests)
        frame = loader.decoder.decode([streams[k]])
        H, W = int(frame.shape[1]), int(frame.shape[2])
        Wr, Hr = rescale_size(W, H, (-1, 24))
        r = bd.kernels.resize_linear_u8(frame, Hr, Wr)[0].cpu().float()
        top, left = (Hr - 20) // 2, (Wr - 20) // 2
        crop = r[top:top + 20, left:left + 20].permute(2, 0, 1)
        mean, inv = torch.tensor(bd.frontend.IMG_MEAN).view(3, 1, 1), 1.0 / torch.tensor(bd.frontend.IMG_STD).view(3, 1, 1)
        assert torch.equal(got[k, 3].cpu(), (crop - mean) * inv), k
