"""Gradient accumulation over several ranks (``accumulate_grad_batches > 1`` under data parallelism; the reference hands both to one
``pl.Trainer``, libs/cil/cil.py:748,:779): ``GradAllReducer.set_sync(False)`` / ``no_sync()`` lets a micro-batch accumulate into ``p.grad``
without any collective, the last micro-batch of an optimizer step reduces the accumulated gradients, one all-reduce per bucket.
gloo, world 2, on CPU, spawned as tests/test_ddp_cpu.py spawns its workers."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


class _Toy(nn.Module):
    """An MLP with a side branch that the caller can leave out of a forward pass."""

    def __init__(self):
        super().__init__()
        self.a, self.side, self.b, self.c = nn.Linear(12, 32), nn.Linear(12, 32), nn.Linear(32, 32), nn.Linear(32, 5)

    def forward(self, x, use_side=True):
        h = self.a(x)
        if use_side:
            h = h + self.side(x)
        return self.c(torch.relu(self.b(torch.relu(h))))


def _data():
    g = torch.Generator().manual_seed(123)
    return torch.randn(8, 12, generator=g), torch.randint(0, 5, (8,), generator=g)


def _micro(rank, k):
    """Micro-batch k (0, 1) of ``rank``: rows of the 8-sample full batch."""
    lo = 4 * rank + 2 * k
    return slice(lo, lo + 2)


BUCKET_MB = 0.002          # 2 KB buckets: the 2085-parameter toy (8.3 KB) fills several


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bdvcil_amd as bd
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.manual_seed(0)
    model = _Toy()
    bd.broadcast_parameters(model)
    reducer = bd.GradAllReducer(model, bucket_cap_mb=BUCKET_MB, tail_cap_mb=0)
    calls = []
    real = dist.all_reduce

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    dist.all_reduce = counting
    x, y = _data()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    per_step, first = [], None
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        before = len(calls)
        for k in range(2):
            sl = _micro(rank, k)
            loss = nn.functional.cross_entropy(model(x[sl], use_side=(k == 0)), y[sl]) / 2
            if k == 0:
                with reducer.no_sync():         # the side branch gets its only gradient here
                    loss.backward()
                assert len(calls) == before
            else:
                reducer.set_sync(True)
                loss.backward()
        reducer.finish()
        per_step.append(len(calls) - before)
        if step == 0:
            first = {n: (p.grad * reducer.grad_scale).clone().numpy() for n, p in model.named_parameters()}
        with torch.no_grad():                   # the mean over ranks, as FusedSGD.set_grad_scale applies it
            for p in model.parameters():
                p.grad.mul_(reducer.grad_scale)
        opt.step()
    dist.all_reduce = real
    q.put((rank, first, per_step, len(reducer.buckets), {n: p.detach().clone().numpy() for n, p in model.named_parameters()}))
    dist.barrier()
    dist.destroy_process_group()


def test_accumulated_gradients_one_allreduce_per_bucket():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, g0, steps0, nb0, w0), (_, g1, steps1, nb1, w1) = res
    assert nb0 == nb1 and nb0 >= 2
    # exactly one all-reduce per bucket per optimizer step, on both ranks
    assert steps0 == [nb0] * 3 and steps1 == [nb0] * 3
    # the reference: the four micro-batches as one full batch on one process (mean of the four micro-batch losses)
    torch.manual_seed(0)
    model = _Toy()
    x, y = _data()
    loss = sum(nn.functional.cross_entropy(model(x[_micro(r, k)], use_side=(k == 0)), y[_micro(r, k)]) for r in range(2) for k in range(2)) / 4
    loss.backward()
    for n, p in model.named_parameters():
        assert torch.allclose(torch.from_numpy(g0[n]), p.grad, rtol=1e-6, atol=1e-7), n
        assert (g0[n] == g1[n]).all(), n
    # the parameter used only in the first (unsynchronised) micro-batch carries its summed gradient
    assert abs(g0['side.weight']).max() > 0
    # weights bit-equal across ranks after 3 optimizer steps
    for n in w0:
        assert (w0[n] == w1[n]).all(), n


def test_fit_epochs_marks_the_boundary_micro_batches():
    """``CILTaskLoop._fit_epochs`` with ``accumulate_grad_batches=2`` and a reducer: 5 batches -> the reducer is told to skip micro-batches
    0 and 2, to reduce 1, 3 and the epoch's last one (4, a step of its own), and ``finish()`` runs once per optimizer step, after the
    backward it belongs to.  The loop is driven on CPU stand-ins: no model of the package, no process group."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bdvcil_amd.task_loop as TL
    events = []

    class Reducer:
        def set_sync(self, flag):
            events.append(('sync', bool(flag)))

        def finish(self):
            events.append(('finish',))

    class Loop(TL.CILTaskLoop):
        def __init__(self):                                   # no files, no models: only what _fit_epochs reads
            self.config = TL.AttrDict(videos_per_gpu=2)
            self._shuffle_gen = torch.Generator().manual_seed(0)
            self.rank, self.world, self._prefetcher = 0, 1, None
            self.current_model = nn.Linear(3, 1)
            self.clip_loader = lambda infos, phase: {'x': torch.ones(len(infos), 3)}

        def _training_step(self, batch):
            loss = self.current_model(batch['x']).sum()
            loss.register_hook(lambda g: events.append(('backward',)))
            return {'loss': loss}

    loop = Loop()
    records = TL.RawframeRecords(None, None)
    records.video_infos = [dict(frame_dir=f'v{i}', total_frames=8, label=0) for i in range(9)]       # 5 batches of <= 2
    opt = torch.optim.SGD(loop.current_model.parameters(), lr=0.1)
    steps = []
    real_step = opt.step
    opt.step = lambda: (events.append(('step',)), real_step())[1]
    losses = []
    loop._fit_epochs(records, 1, False, opt, None, Reducer(), None, 2, losses)
    assert len(losses) == 1
    micro = [('sync', False), ('backward',)]
    last = [('sync', True), ('backward',), ('finish',), ('step',)]
    assert events == micro + last + micro + last + last
