"""Step, conv and scale-pass time of the conv arithmetics that keep fp32 tensors, on the bench workload (TSM-R50, 32 clips of
8 x 224 x 224, forward + backward + SGD): 'bf16x3' (the default), 'bf16x2' and 'f16x2'.  The modes run in interleaved rounds in ONE
process on one build and one model (timings from separate processes or boxes differ by more than some of the effects).  Prints one
line per mode: ms per step of every round, the median, clips/s, its share of the 'bf16x3' median; then, from HIP events around every
conv call of ONE extra step per mode with the side stream off (as bench.py's conv_ms_per_step), the conv time of a step and, of it,
the time of the 'f16x2' scale passes (``kernels.act_amax``: one HBM pass per operand tensor).
    python tools/bench_arith.py [rounds] [steps] [batch] > profiles/f16x2.txt
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bdvcil_amd as bd
from bdvcil_amd import functional as Fn
from bdvcil_amd import kernels as K
from bench import ConvTimer, model_cfg

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = int(sys.argv[3]) if len(sys.argv) > 3 else 32
dev = torch.device('cuda:0')
MODES = ('bf16x3', 'bf16x2', 'f16x2')
OPT = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01,
           momentum=0.9, weight_decay=1e-4)

g = torch.Generator().manual_seed(1000)
batch = dict(imgs=torch.randn(B, 8, 3, 224, 224, generator=g).to(dev), label=torch.randint(0, 101, (B, 1), generator=g).to(dev))
torch.manual_seed(0)
model = bd.build_model(model_cfg(50, 101, 'SimpleLinear', 'CrossEntropyLoss', 0.5)).to(dev)
model.train()
engine = bd.TrainEngine(model, bd.build_optimizer(model, OPT))

# event pairs around the scale passes (they run inside the conv calls, so their time is part of the conv time below)
amax_records = []
amax_words = {}         # id(word) -> word: the words seen on the timed step (held, so that the ids stay theirs)
amax_on = False
inner_amax = K.act_amax


def timed_amax(t):
    if not amax_on:
        return inner_amax(t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = inner_amax(t)
    e1.record()
    if id(out) not in amax_words:       # a new word: the pass ran (a cached word costs no launch)
        amax_words[id(out)] = out
        amax_records.append((e0, e1))
    return out


K.act_amax = timed_amax
timer = ConvTimer()
timer.wrap(K)


def run(mode, n):
    K.set_conv_arith(mode)
    for _ in range(2):
        engine.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        engine.step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def conv_times(mode):
    """(conv ms, scale-pass ms, scale passes) of one step, side stream off: an event pair then brackets the call's kernels alone."""
    global amax_on
    K.set_conv_arith(mode)
    for _ in range(2):
        engine.step(batch)
    was = Fn.side_stream_enabled()
    Fn.set_side_stream_enabled(False)
    try:
        torch.cuda.synchronize()
        timer.records, timer.enabled, amax_on = [], True, True
        del amax_records[:]
        amax_words.clear()
        K._AMAX.clear()                 # words of the warm-up steps' tensors that are still alive
        engine.step(batch)
        torch.cuda.synchronize()
    finally:
        timer.enabled = amax_on = False
        Fn.set_side_stream_enabled(was)
    conv = sum(v['ms'] for v in timer.summary().values())
    return conv, sum(a.elapsed_time(b) for a, b in amax_records), len(amax_records)


times = {m: [] for m in MODES}
try:
    for r in range(rounds):
        for m in MODES:
            times[m].append(run(m, steps))
    conv = {m: conv_times(m) for m in MODES}
finally:
    K.set_conv_arith('bf16x3')
med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
base = med['bf16x3']
print(f'# TSM-R50, B={B}, T=8, 224x224, fwd + bwd + SGD; {rounds} interleaved rounds of {steps} steps, one process, one model, '
      f'{torch.cuda.get_device_name(0)}')
for m in MODES:
    c, s, n = conv[m]
    print(f'{m:7s} ' + ' '.join(f'{t:7.2f}' for t in times[m]) + f'   median {med[m]:7.2f} ms/step  ({B * 1e3 / med[m]:6.1f} clips/s)  '
          f'{100 * med[m] / base:5.1f} % of bf16x3   conv {c:6.2f} ms/step (one step, side stream off), of it scale passes {s:5.2f} ms '
          f'in {n} launches')
