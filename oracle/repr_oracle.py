"""CPU oracle for the inference + representation path -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Restates, in plain torch on the CPU, the reference arithmetic that ``csrc/repr.hip`` implements:

* ``predict_repr``        libs/cil/cil.py:501-506 (_extract_repr) and :564-571 (predict_step, extract_repr)
* ``nme_classify``        libs/cil/cil.py:945-960
* ``class_means``         libs/cil/cil.py:1079-1083
* ``herding_select``      libs/cil/memory_selection.py:70-92 (greedy loop) and :150-164 (calc_mean_features)

Every function computes in the dtype of its inputs: fp32 inputs give the reference's own arithmetic, fp64 inputs the high-precision
restatement that tests/test_repr_edges_gpu.py holds the kernels against (``herding_margin`` / ``argmax_margin`` say how far a selection
is from flipping; ``softmax_mean`` / ``topk_hit_counts`` restate the two evaluation kernels of csrc/head_loss.hip).

Pinning: ``herding_select`` is checked against ``tests/golden/herding_golden.npz``, produced by the reference's own
``Herding.construct_exemplar`` (tests/golden/make_golden_herding.py).  The three cil.py snippets live inside a
LightningModule that cannot be imported here (pytorch_lightning / mmaction absent): they are a handful of torch calls
(``F.normalize``, ``F.cosine_similarity``, ``mean``, ``argmax``) restated verbatim -- parity unpinned beyond torch itself.
"""
from typing import Tuple

import torch
import torch.nn.functional as F


def predict_repr(pooled: torch.Tensor, batch_size: int, num_segments: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """pooled: hooked ``cls_head.avg_pool`` output (B*crops*T, D, 1, 1) or (B*crops*T, D)."""
    repr_ = pooled.flatten(1)
    repr_ = repr_.view(-1, num_segments, repr_.size(1))
    repr_consensus = repr_.mean(dim=1, keepdim=True).squeeze(1)          # AvgConsensus(dim=1)
    embedding_size = repr_consensus.size(-1)
    r = repr_consensus.view(batch_size, -1, embedding_size)             # (batch_size, num_crops, dim)
    r = F.normalize(r, p=2, dim=-1)
    return r, torch.mean(r, dim=1, keepdim=False)


def nme_classify(repr_: torch.Tensor, exemplar_class_means: torch.Tensor):
    num_samples, num_crops, _ = repr_.shape
    r = repr_.reshape(-1, repr_.size(2))
    num_classes = exemplar_class_means.size(0)
    size, dims = r.shape
    repr_broadcast = r.unsqueeze(dim=1).expand(size, num_classes, dims)
    similarity = F.cosine_similarity(repr_broadcast, exemplar_class_means, dim=-1)
    similarity = torch.mean(similarity.reshape(num_samples, num_crops, num_classes), dim=1, keepdim=False)
    return similarity, torch.argmax(similarity, dim=1, keepdim=False)


def class_means(mean_crops_repr: torch.Tensor, label: torch.Tensor, num_classes: int) -> torch.Tensor:
    r = mean_crops_repr.reshape(-1, mean_crops_repr.size(-1))
    out = []
    for class_idx in range(num_classes):
        indices = (label == class_idx).nonzero().squeeze(dim=1)
        out.append(torch.mean(r[indices], dim=0))
    return torch.stack(out, dim=0)


def _remove_row(t: torch.Tensor, idx) -> torch.Tensor:
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[idx] = False
    return t[keep]


def herding_trace(features: torch.Tensor, num_exemplars: int, cosine_distance: bool):
    """The greedy loop in the dtype of ``features`` -> (class_mean (1, dims), indices, dist, steps); ``steps[i]`` holds the distances
    of every row still available at step i, ascending."""
    if cosine_distance:
        normalized = F.normalize(features, p=2, dim=-1)
    else:
        normalized = features
    mean = features.view(-1, features.size(-1)).mean(0, keepdim=True)
    class_mean = F.normalize(mean, p=2) if cosine_distance else mean
    indexer = torch.arange(features.size(0))
    moving = torch.zeros(1, features.size(-1), dtype=features.dtype)
    indices, dists, steps = [], [], []
    for n in range(1, num_exemplars + 1):
        tmp = moving * (n - 1) / n + normalized / n
        if cosine_distance:
            dist = 1 - torch.cosine_similarity(tmp, class_mean, dim=1)
        else:
            dist = torch.pairwise_distance(tmp, class_mean.squeeze(dim=0), p=2)
        row = torch.argmin(dist)
        moving = moving * (n - 1) / n + normalized[row] / n
        indices.append(indexer[row].item())
        dists.append(dist[row].item())
        steps.append(torch.sort(dist).values)
        normalized = _remove_row(normalized, row)
        indexer = _remove_row(indexer, row)
    return class_mean, indices, dists, steps


def herding_select(features: torch.Tensor, num_exemplars: int, cosine_distance: bool):
    """features (n, dims) of one class -> (class_mean (1, dims), indices, dist), in the dtype of ``features``."""
    return herding_trace(features, num_exemplars, cosine_distance)[:3]


def herding_margin(features: torch.Tensor, num_exemplars: int, cosine_distance: bool, distinct: bool = False):
    """fp64: (smallest gap between the best and the second-best distance over all greedy steps, largest selected distance).  A step
    with one row left has no runner-up and does not count.  ``distinct``: the runner-up is the nearest row at a *different*
    distance, for inputs with a planted duplicate row (whose distance is bit-identical in any arithmetic)."""
    _, _, dists, steps = herding_trace(features.double(), num_exemplars, cosine_distance)
    gap = float('inf')
    for d in steps:
        rest = d[d > d[0]] if distinct else d[1:]
        if rest.numel():
            gap = min(gap, (rest[0] - d[0]).item())
    return gap, max(dists, default=0.0)


def argmax_margin(sim: torch.Tensor) -> torch.Tensor:
    """Per row: best minus second-best value (inf for a single column)."""
    if sim.size(1) < 2:
        return torch.full((sim.size(0),), float('inf'), dtype=sim.dtype)
    top = torch.topk(sim, 2, dim=1).values
    return top[:, 0] - top[:, 1]


def softmax_mean(s: torch.Tensor, B: int, n: int, apply_softmax: bool) -> torch.Tensor:
    """average_clip in fp64: s (B*n, K) -> (B, K), the mean over n of the (softmaxed) rows."""
    s = s.double().view(B, n, -1)
    return (torch.softmax(s, dim=2) if apply_softmax else s).mean(dim=1)


def topk_hit_counts(score, labels, ks=(1, 5)):
    """NumPy: for each k the number of rows whose label has fewer than k classes scoring strictly higher (ties are not higher)."""
    import numpy as np
    score, labels = np.asarray(score), np.asarray(labels)
    greater = (score > score[np.arange(score.shape[0]), labels][:, None]).sum(axis=1)
    return tuple(int((greater < k).sum()) for k in ks)


def herding_class_features(features: torch.Tensor, storing_methods: str) -> torch.Tensor:
    """memory_selection.py:50-69: per-class feature tensor -> (n, dims)."""
    if storing_methods == 'videos':
        return features.squeeze(dim=1) if features.size(1) == 1 else features.mean(1)
    if storing_methods == 'clips':
        features = features.view(-1, features.size(2), features.size(3))
        if features.size(1) == 1:
            return features.squeeze(dim=1)
        # Reference quirk (:63-69): the tensor is already 3-D (videos x clips, samples, dims) here, so ``mean(2)``
        # averages over the feature dimension and herding then runs on (videos x clips, samples) vectors.
        features = features.mean(2)
        return features.view(-1, features.size(-1))
    raise NotImplementedError
