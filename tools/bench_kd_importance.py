"""Times of the time-channel importance kernels (csrc/tc_kd.hip) at the five KD tensors of TSM-R50 with B = 32, T = 8 --
(256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7) and the pooled (256, 2048, 1, 1).

Weighted loss, fp32 and bf16 storage, forward + backward through autograd:

  new   ``functional.kd_time_channel`` with a random (T, C) map
  mse   ``functional.kd_mse``, the loss it weights (csrc/head_loss.hip)

Accumulate pass, fp32 gradients:

  new    ``kernels.tc_sqgrad_accum``
  torch  ``(g * g).view(B, T, C, -1).sum((0, 3)) * B^2`` added to S, on the channels-last view the backward hands over

The forms are timed interleaved in one process: ``--rounds`` times, ``--iters`` back-to-back calls of each form between two device
events; the median round is reported with the fastest and the slowest.  The maps are channels-last views, as the hooked stage
outputs are.  Bytes are the algorithm's, computed from the shapes here: with M the bytes of one map, both losses move 2 M forward
and 3 M backward (the (T, C) table, at most 64 KB, stays in cache); the accumulate pass reads the gradient once, M.

``--estimator``: one batch of ``estimate_kd_importance`` on TSM-R50 (B clips of 8 x 224 x 224, the five KD modules) against one
training step (forward + backward + SGD) of the same model and batch, interleaved; the estimation visits every record of a task
once, a task trains ``--epochs`` epochs on them, so its share of the task's GPU time is r / (epochs + r) with r the ratio of the two.
Information only: nothing in the suite depends on these numbers.

    python tools/bench_kd_importance.py [--frames 256] [--iters 20] [--rounds 7] [--estimator] [--batch 32] [--epochs 50]
                                        [--out profiles/kd_importance.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(256, 56, 56), (512, 28, 28), (1024, 14, 14), (2048, 7, 7), (2048, 1, 1)]      # (C, H, W) per frame
KD_NAMES = ['backbone.layer1', 'backbone.layer2', 'backbone.layer3', 'backbone.layer4', 'cls_head.avg_pool']
T = 8


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--estimator', action='store_true')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import bdvcil_amd as bd
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_kd_importance.py needs a GPU: a CPU run gives no time')
    K, Fn = bd.kernels, bd.functional
    dev = torch.device('cuda:0')
    N = args.frames
    if N % T:
        raise SystemExit(f'--frames must be a multiple of {T}')
    lines = [f'time-channel importance distillation, N={N} frames, T={T}, {args.rounds} interleaved rounds of {args.iters} calls '
             f'(device events; median [min .. max] us per call); losses fwd+bwd through autograd unless marked']

    def timed(fn, iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / iters

    def stat(ts):
        return f'{statistics.median(ts):8.1f} [{min(ts):8.1f} .. {max(ts):8.1f}] us'

    def measure(forms, iters):
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                times[k].append(timed(fn, iters))
        return times, {k: statistics.median(v) for k, v in times.items()}

    for storage, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        for C, H, W in SIZES:
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.relu(torch.randn(N, H, W, C, device=dev, generator=g))
            y = torch.relu(x + 0.3 * torch.randn(N, H, W, C, device=dev, generator=g))
            cur = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)         # channels-last views, as the hooks return them
            prev = y.to(dtype).permute(0, 3, 1, 2)
            del x, y
            A = torch.rand(T, C, device=dev, generator=g) + 0.1
            A = (A / A.mean()).contiguous()
            one = torch.ones(1, device=dev)

            def run(fn):
                cur.grad = None
                fn().backward()

            forms = {'new': lambda: run(lambda: Fn.kd_time_channel(cur, prev, A)), 'mse': lambda: run(lambda: Fn.kd_mse(cur, prev)),
                     'new fwd only': lambda: K.kd_tc_fwd(cur.detach(), prev, A), 'mse fwd only': lambda: K.kd_mse_fwd(cur.detach(), prev),
                     'new bwd only': lambda: K.kd_tc_bwd(cur.detach(), prev, A, one),
                     'mse bwd only': lambda: K.kd_mse_bwd(cur.detach(), prev, one, 1.0)}
            times, med = measure(forms, args.iters)
            M = cur.numel() * cur.element_size()
            head = f'{storage} ({N}, {C}, {H}, {W}) map {M / 1e6:7.1f} MB'
            lines.append(f'{head} | new {stat(times["new"])} | mse {stat(times["mse"])} | {5 * M / 1e6:7.1f} MB each | new/mse {med["new"] / med["mse"]:5.2f}')
            print(lines[-1], flush=True)
            for k, by in (('fwd only', 2 * M), ('bwd only', 3 * M)):
                lines.append(f'{"":>{len(head)}} | new {k} {stat(times["new " + k])} {by / med["new " + k] / 1e6:5.2f} TB/s | '
                             f'mse {k} {stat(times["mse " + k])} {by / med["mse " + k] / 1e6:5.2f} TB/s | new/mse {med["new " + k] / med["mse " + k]:5.2f}')
                print(lines[-1], flush=True)
            if dtype == torch.float32:
                B = N // T
                grad = cur.detach()
                S1, S2 = torch.zeros(T, C, device=dev), torch.zeros(T, C, device=dev)
                acc = {'new': lambda: K.tc_sqgrad_accum(S1, grad, float(B)),
                       'torch': lambda: S2.add_((grad * grad).reshape(B, T, C, -1).sum(dim=(0, 3)) * float(B * B))}
                times, med = measure(acc, args.iters)
                lines.append(f'{"":>{len(head)}} | accumulate new {stat(times["new"])} {M / 1e6:7.1f} MB {M / med["new"] / 1e6:5.2f} TB/s | '
                             f'torch {stat(times["torch"])} | torch/new {med["torch"] / med["new"]:5.2f}')
                print(lines[-1], flush=True)
                del grad, acc
            del cur, prev, forms
            torch.cuda.empty_cache()
    lines.append('note: every call of a window touches the same buffers; maps up to the 256 MiB Infinity Cache (all but the fp32 and bf16 layer-1 '
                 'and the fp32 layer-2 maps) are served partly from it, so their rates may exceed what HBM alone delivers; the forms of a '
                 'line run under the same conditions.  fwd+bwd includes the autograd node, the allocation of dcur and the host checks.')

    if args.estimator:
        from bench import model_cfg
        B = args.batch
        torch.manual_seed(0)
        model = bd.build_model(model_cfg(50, 101, 'SimpleLinear', 'CrossEntropyLoss', 0.5)).to(dev)
        model.train()
        opt = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01,
                   momentum=0.9, weight_decay=1e-4)
        engine = bd.TrainEngine(model, bd.build_optimizer(model, opt))
        g = torch.Generator().manual_seed(1000)
        batch = dict(imgs=torch.randn(B, T, 3, 224, 224, generator=g).to(dev), label=torch.randint(0, 101, (B, 1), generator=g).to(dev))
        forms = {'estimate': lambda: bd.estimate_kd_importance(model, [batch], KD_NAMES, T), 'train step': lambda: engine.step(batch)}
        times, med = measure(forms, max(1, args.iters // 4))
        r = med['estimate'] / med['train step']
        lines.append(f'estimator, TSM-R50, B={B}, T={T}, 224x224, modules {KD_NAMES}: one batch of estimate_kd_importance '
                     f'{stat(times["estimate"])} | one training step (fwd + bwd + SGD) {stat(times["train step"])} | ratio {r:5.2f} | '
                     f'share of a task of {args.epochs} epochs {100 * r / (args.epochs + r):5.2f} %')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
