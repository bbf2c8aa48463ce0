"""Device-event times of the step-tail kernels that use the pieces of csrc/reduce_pieces.h, each through its kernels.py wrapper at the
workload's size: the heads at (256, 2048) x 101 (LSC with 3 proxies), the losses at B 32, the distillation losses on the TSM-R50
layer-1 to layer-4 maps at B 32, T 8 in fp32 and bf16 storage (channels-last views, as the hooks return them), the squared gradient
norm over the ResNet-50 parameter list, and the NME classifier and the herding loop at 2048 features.  20 back-to-back calls between
two device events, the median of five such windows, microseconds per call; prints one JSON line.  The library is the one
``BDVCIL_LIB_PATH`` names (unset: this tree's), so two builds are compared by running the tool once per library, alternating
(profiles/tail_kernel_dedupe.txt).  tools/bench_pod_kd.py and tools/bench_kd_importance.py time the same distillation kernels
beside their torch composites and print text; this tool times the wrappers alone.  Information only: nothing in the suite depends on
these numbers.

    [BDVCIL_LIB_PATH=other/libbdvcil_hip.so] python tools/bench_tail_kernels.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdvcil_amd import kernels as K             # noqa: E402
from bdvcil_amd.optim import FusedSGD           # noqa: E402

MAPS = [('layer1', 256, 56, 56), ('layer2', 512, 28, 28), ('layer3', 1024, 14, 14), ('layer4', 2048, 7, 7)]     # (C, H, W) per frame


def timeit(fn, iters=20, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / iters * 1000.0)
    return round(float(np.median(best)), 2)


def r50_shapes(num_classes=101):
    """Parameter shapes of a ResNet-50 with a linear head: conv weights and the weight / bias of their BatchNorms."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    cin = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            for co, ci, k in ((width, cin, 1), (width, width, 3), (4 * width, width, 1)) + (((4 * width, cin, 1),) if b == 0 else ()):
                shapes += [(co, ci, k, k), (co,), (co,)]
            cin = 4 * width
    return shapes + [(num_classes, 2048), (num_classes,)]


def main():
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cuda').manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)                                  # noqa: E731
    res = {'lib': os.environ.get('BDVCIL_LIB_PATH', 'new')}
    N, D, Kc, P, B, T = 256, 2048, 101, 3, 32, 8
    x, w, wl, bl, dsim = rn(N, D), rn(Kc, P * D), rn(Kc, D), rn(Kc), rn(N, Kc)
    sim, xnorm, wnorm, cosbuf = K.lsc_fwd(x, w, Kc, P)
    res['lsc_fwd_us'] = timeit(lambda: K.lsc_fwd(x, w, Kc, P))
    res['lsc_bwd_us'] = timeit(lambda: K.lsc_bwd(dsim, x, w, xnorm, wnorm, cosbuf, Kc, P))
    res['linear_fwd_us'] = timeit(lambda: K.linear_fwd(x, wl, bl))
    score, labels, eta = rn(B, Kc), torch.randint(0, Kc, (B,), device=dev, generator=g), torch.ones(1, device=dev)
    res['lsc_loss_us'] = timeit(lambda: K.lsc_loss(score, labels, eta, 0.0, True))
    res['topk_acc_us'] = timeit(lambda: K.topk_acc(score, labels))
    one = torch.ones(1, device=dev)
    A = None
    for storage, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        for name, C, H, W in MAPS:
            cur = torch.relu(rn(B * T, H, W, C)).to(dtype).permute(0, 3, 1, 2)
            prev = torch.relu(rn(B * T, H, W, C)).to(dtype).permute(0, 3, 1, 2)
            A = torch.rand(T, C, device=dev, generator=g) + 0.5
            res[f'kd_mse_fwd_{name}_{storage}_us'] = timeit(lambda: K.kd_mse_fwd(cur, prev))
            res[f'kd_tc_fwd_{name}_{storage}_us'] = timeit(lambda: K.kd_tc_fwd(cur, prev, A))
            res[f'pod_spatial_fwd_{name}_{storage}_us'] = timeit(lambda: K.pod_spatial_fwd(cur, prev))
            del cur, prev
            torch.cuda.empty_cache()
    params = [torch.nn.Parameter(rn(*s)) for s in r50_shapes()]
    for p in params:
        p.grad = rn(*p.shape)
    opt = FusedSGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4)
    t = opt._build_tables(opt._active())
    sq = torch.zeros(1, device=dev)
    res['multi_sqnorm_r50_us'] = timeit(lambda: K.multi_sqnorm(t['g'], t['n'], len(params), sq))
    rp, means = rn(B, 3, D), rn(Kc, D)
    res['nme_classify_us'] = timeit(lambda: K.nme_classify(rp, means))
    feats = rn(100, D)
    res['herding_select_100x20_us'] = timeit(lambda: K.herding_select(feats, 20, True), iters=5)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
