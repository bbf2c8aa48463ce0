"""numpy oracle of the person-masked temporal median (``bdv_temporal_masked_median_u8``) and the stacks and
box tables the tests feed it.  Not a test module: ``oracle/`` is frozen, so the helper lives here.

Per video and pixel: S = the frames none of whose boxes contains the pixel (``x0 <= x < x1 and y0 <= y < y1``); ``visible = |S|``;
each channel is ``np.median`` over S, ``.astype(np.uint8)``, when ``|S| >= min_visible``, else ``np.median`` over all frames."""
import numpy as np


def covered(boxes_per_frame, H, W):
    """(F, H, W) bool: ``mask[y0:y1, x0:x1] = True`` per box row, BuildHumanMask's form."""
    cov = np.zeros((len(boxes_per_frame), H, W), dtype=bool)
    for f, rows in enumerate(boxes_per_frame):
        for x0, y0, x1, y1 in np.asarray(rows, dtype=np.int64).reshape(-1, 4):
            cov[f, y0:y1, x0:x1] = True
    return cov


def masked_median(stack, boxes_per_frame, min_visible=1):
    """``stack`` (F, H, W, 3) uint8, ``boxes_per_frame`` F arrays of (n, 4) rows -> ``(out (H, W, 3) uint8, visible (H, W) uint16)``.
    Pixel by pixel: the uncovered samples are collected in a Python loop and handed to ``np.median``."""
    F, H, W, _ = stack.shape
    out = np.empty((H, W, 3), dtype=np.uint8)
    visible = np.empty((H, W), dtype=np.uint16)
    for y in range(H):
        for x in range(W):
            keep = [f for f in range(F)
                    if not any(r[0] <= x < r[2] and r[1] <= y < r[3] for r in np.asarray(boxes_per_frame[f]).reshape(-1, 4))]
            visible[y, x] = len(keep)
            samples = stack[keep, y, x] if len(keep) >= min_visible else stack[:, y, x]
            out[y, x] = np.median(samples.astype(np.float64), axis=0).astype(np.uint8)
    return out, visible


def masked_median_grouped(stack, boxes_per_frame, min_visible=1):
    """The same result for frames too large for the pixel loop: the pixels are grouped by the set of frames that cover them (few
    boxes make few distinct sets) and ``np.median`` runs once per group.  The tests check it against ``masked_median`` where both run."""
    F, H, W, _ = stack.shape
    cov = covered(boxes_per_frame, H, W).reshape(F, H * W)
    flat = stack.reshape(F, H * W, 3)
    out = np.empty((H * W, 3), dtype=np.uint8)
    patterns, group = np.unique(cov, axis=1, return_inverse=True)
    group = np.asarray(group).reshape(-1)
    for g in range(patterns.shape[1]):
        keep = ~patterns[:, g]
        px = np.flatnonzero(group == g)
        samples = flat[keep][:, px] if keep.sum() >= min_visible else flat[:, px]
        out[px] = np.median(samples.astype(np.float64), axis=0).astype(np.uint8)
    return out.reshape(H, W, 3), (F - cov.sum(0)).astype(np.uint16).reshape(H, W)


def box_table(videos_boxes):
    """``videos_boxes``: per video a list of per-frame (n, 4) rows -> the CSR table over the batch's frames ``(box_first, boxes)``."""
    first, rows = [0], []
    for boxes_per_frame in videos_boxes:
        for r in boxes_per_frame:
            r = np.asarray(r, dtype=np.int32).reshape(-1, 4)
            rows.append(r)
            first.append(first[-1] + len(r))
    return np.asarray(first, dtype=np.int32), (np.concatenate(rows) if rows else np.zeros((0, 4), np.int32)).astype(np.int32)


def value_stack(family, F, H, W, rng):
    """The value families of tests/test_background_gpu.py: uniform noise, the narrow band 100..103, and stacks whose two middle
    values straddle a high-nibble boundary (even F)."""
    shape = (F, H, W, 3)
    if family == 'noise':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if family == 'narrow':
        return rng.integers(100, 104, shape, dtype=np.uint8)
    lo, hi = {'mid15_16': (15, 16), 'mid127_128': (127, 128)}[family]
    assert F % 2 == 0
    s = np.empty(shape, dtype=np.uint8)
    s[:F // 2] = lo
    s[F // 2:] = hi
    if F > 2:
        s[0] = rng.integers(0, lo + 1, shape[1:])
        s[-1] = rng.integers(hi, 256, shape[1:])
    return s[rng.permutation(F)]


def edge_boxes(F, H, W, whole_first):
    """Per-frame box rows of an F-frame video (H >= 5, W >= 6) that make, for F >= 7, pixels seen in 0, 1, 2 and 3 frames:

      every frame but the first   [0, 0, 2, 2]          a person who never moves; with ``whole_first`` those pixels are seen in no frame
      frame 0, ``whole_first``    [0, 0, W, H]          one box covers a whole frame
      frame 1                     [1, 1, 4, 3] and [2, 2, 5, 4] overlap; [3, 3, 3, 5] has zero area
      frames 1 .. F-2             column x = 2          seen in the last frame (and in frame 0 without ``whole_first``)
      frames 1 .. F-3             column x = 4          one frame more
      frames 1 .. F-4             column x = 3          one frame more

    The box edges x = 2, 3, 4, 5 in row 0 lie inside lanes 1, 2, 3 (bytes 4-7, 8-11, 12-15 hold pixels 1|2, 2|3, 4|5 ...), so a
    boundary falls between the two pixels that share a lane's 4 bytes."""
    out = []
    for f in range(F):
        rows = []
        if f == 0 and whole_first:
            rows.append([0, 0, W, H])
        if f >= 1:
            rows.append([0, 0, 2, 2])
        if f == 1:
            rows += [[1, 1, 4, 3], [2, 2, 5, 4], [3, 3, 3, 5]]
        if 1 <= f <= F - 2:
            rows.append([2, 0, 3, H])
        if 1 <= f <= F - 3:
            rows.append([4, 0, 5, H])
        if 1 <= f <= F - 4:
            rows.append([3, 0, 4, H])
        out.append(np.asarray(rows, dtype=np.int32).reshape(-1, 4))
    return out
