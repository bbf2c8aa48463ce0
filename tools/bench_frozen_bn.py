"""Step time and peak memory of the frozen-BatchNorm training modes on the bench workload (TSM-R50, 32 clips of 8 x 224 x 224,
forward + backward + SGD): train-mode BatchNorm, ``norm_eval``, ``partial_bn``, and ``frozen_stages=2`` with ``partial_bn``.  The
modes run in interleaved rounds in ONE process on one build (timings from separate processes or boxes differ by more than some of
the effects).  Prints one line per mode: ms per step of every round, the median, its share of the train-mode median, and
``torch.cuda.max_memory_allocated`` of a step.
    python tools/bench_frozen_bn.py [rounds] [steps] [batch] > profiles/frozen_bn.txt
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bdvcil_amd as bd
from bench import model_cfg

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
dev = torch.device('cuda:0')

MODES = {
    'train-mode BatchNorm': dict(),
    'norm_eval': dict(norm_eval=True),
    'partial_bn': dict(partial_bn=True),
    'frozen_stages=2 + partial_bn': dict(frozen_stages=2, partial_bn=True),
}
OPT = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01,
           momentum=0.9, weight_decay=1e-4)

g = torch.Generator().manual_seed(1000)
batch = dict(imgs=torch.randn(B, 8, 3, 224, 224, generator=g).to(dev), label=torch.randint(0, 101, (B, 1), generator=g).to(dev))
engines = {}
for name, opts in MODES.items():
    torch.manual_seed(0)
    cfg = model_cfg(50, 101, 'SimpleLinear', 'CrossEntropyLoss', 0.5)
    cfg['backbone'].update(opts)
    model = bd.build_model(cfg).to(dev)
    model.train()
    engines[name] = bd.TrainEngine(model, bd.build_optimizer(model, OPT))


def run(engine, n):
    for _ in range(2):
        engine.step(batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        engine.step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated(dev)


times = {k: [] for k in MODES}
peak = {k: 0 for k in MODES}
for r in range(rounds):
    for name, engine in engines.items():
        ms, mem = run(engine, steps)
        times[name].append(ms)
        peak[name] = max(peak[name], mem)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
base = med['train-mode BatchNorm']
print(f'# TSM-R50, B={B}, T=8, 224x224, fwd + bwd + SGD; {rounds} interleaved rounds of {steps} steps, one process, {torch.cuda.get_device_name(0)}')
for name in MODES:
    print(f'{name:30s} ' + ' '.join(f'{t:7.2f}' for t in times[name]) + f'   median {med[name]:7.2f} ms/step  ({B * 1e3 / med[name]:6.1f} clips/s)  '
          f'{100 * med[name] / base:5.1f} % of train mode   peak allocated {peak[name] / 2 ** 30:6.2f} GiB')
