"""Step time and peak memory of I3D-ResNet50 (BASELINE config 4: clips of 32 x 224 x 224, batch 16; forward + backward + SGD) in
three conv arithmetics: the default ``bf16x3``, ``bf16x1`` (one bf16 product, fp32 tensors) and ``bf16`` (the same arithmetic with
activations and their gradients stored as bf16).  One model per mode, same initial weights and batch; the modes run in interleaved
rounds in ONE process on one build (timings from separate processes or boxes differ by more than some of the effects).  Prints one
line per mode: ms per step of every round, the median, its share of the default's median, and ``torch.cuda.max_memory_allocated``
of a step.  A record, not a gate: no test runs it.
    python tools/bench_i3d_arith.py [rounds] [steps] [batch] [frames] [size] >> profiles/i3d_bf16.txt
"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bdvcil_amd as bd

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
B = int(sys.argv[3]) if len(sys.argv) > 3 else 16
T = int(sys.argv[4]) if len(sys.argv) > 4 else 32
S = int(sys.argv[5]) if len(sys.argv) > 5 else 224
dev = torch.device('cuda:0')

MODES = ('bf16x3', 'bf16x1', 'bf16')
OPT = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01,
           momentum=0.9, weight_decay=1e-4)
CFG = dict(type='Recognizer3D',
           backbone=dict(type='ResNet3d', pretrained2d=True, pretrained=None, depth=50, conv1_kernel=(5, 7, 7), conv1_stride_t=2,
                         pool1_stride_t=2, conv_cfg=dict(type='Conv3d'), norm_eval=False,
                         inflate=((1, 1, 1), (1, 0, 1, 0), (1, 0, 1, 0, 1, 0), (0, 1, 0)), zero_init_residual=False),
           cls_head=dict(type='I3DHead', num_classes=101, in_channels=2048, spatial_type='avg', dropout_ratio=0.5, init_std=0.01),
           train_cfg=None, test_cfg=dict(average_clips='prob'))         # configs/_base_/models/i3d_r50.py:1-27

g = torch.Generator().manual_seed(1000)
batch = dict(imgs=torch.randn(B, 1, 3, T, S, S, generator=g).to(dev), label=torch.randint(0, 101, (B, 1), generator=g).to(dev))
torch.manual_seed(0)
base = bd.build_model(copy.deepcopy(CFG)).to(dev)
engines = {}
for mode in MODES:
    model = copy.deepcopy(base).train()
    engines[mode] = bd.TrainEngine(model, bd.build_optimizer(model, OPT))


def loss_fn(m, b):
    out = m(b['imgs'], b['label'])
    out['loss'] = out['loss_cls']
    return out


def run(mode, n):
    engine = engines[mode]
    with bd.conv_arith(mode):
        for _ in range(2):
            engine.step(batch, loss_fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            out = engine.step(batch, loss_fn)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated(dev), float(out['loss_cls'].detach())


times = {k: [] for k in MODES}
peak = {k: 0 for k in MODES}
loss = {}
for r in range(rounds):
    for mode in MODES:
        ms, mem, loss[mode] = run(mode, steps)
        times[mode].append(ms)
        peak[mode] = max(peak[mode], mem)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f'# I3D-R50, B={B}, T={T}, {S}x{S}, fwd + bwd + SGD; {rounds} interleaved rounds of {steps} steps (2 warm-up steps each), one process, '
      f'{torch.cuda.get_device_name(0)}')
for mode in MODES:
    print(f'{mode:8s} ' + ' '.join(f'{t:7.2f}' for t in times[mode]) + f'   median {med[mode]:7.2f} ms/step  ({B * 1e3 / med[mode]:6.1f} clips/s)  '
          f'{100 * med[mode] / med["bf16x3"]:5.1f} % of bf16x3   peak allocated {peak[mode] / 2 ** 30:6.2f} GiB   last loss {loss[mode]:.4f}')
