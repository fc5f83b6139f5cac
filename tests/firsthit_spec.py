"""What the first-hit buffers must hold, from the oracle's own camera rays and hit records: the frame's running mean in float32, the geometry channels of
crh_render_aov, the rectangles the dispatch-decomposition tests cut a frame into, and crh_ids_resolve's ranking (a specification: no test lives here;
tests/test_aov.py, tests/test_idmatte.py, the graph tests and the EXR tests use it)."""
import numpy as np

SLOTS, WORDS, LOST, TOTAL = 6, 16, 12, 13          # an ID record (include/cray_hip.h): six ids, six counts, the lost samples, the total


def fold(mean, sample, completed):
    """renderer.c:288-291 in float32, the operations in the reference's order."""
    n1, t = np.float32(completed - 1), np.float32(1.0) / np.float32(completed)
    return ((mean * n1) + sample) * t


def first_hits(oracle, oscene, w, h, passes, max_passes, region=None):
    """oracle.camera_ray -> oracle.trace_rays for every pixel of the region and every pass: hits[pass][row, col] (stored rows run top-down)."""
    x0, y0, x1, y1 = region or (0, 0, w, h)
    rays = np.zeros((len(passes), y1 - y0, x1 - x0, 6), np.float32)
    for k, p in enumerate(passes):
        for y in range(y0, y1):
            for x in range(x0, x1):
                rays[k, y1 - 1 - y, x - x0] = oracle.camera_ray(oscene, x, y, p, max_passes)
    return oracle.trace_rays(oscene, rays.reshape(-1, 6)).reshape(len(passes), y1 - y0, x1 - x0)


def geometry_expected(hits, passes):
    """Channels 3..7 of the samples (a miss: zeros; a hit: the record's normal and distance, coverage 1), folded in pass order."""
    mean = np.zeros(hits.shape[1:] + (5,), np.float32)
    for k, p in enumerate(passes):
        hit = hits[k]["inst"] >= 0
        s = np.zeros_like(mean)
        s[..., 0:3] = np.where(hit[..., None], hits[k]["normal"], np.float32(0))
        s[..., 3] = np.where(hit, hits[k]["distance"], np.float32(0))
        s[..., 4] = hit.astype(np.float32)
        mean = fold(mean, s, p + 1)
    return mean


def ragged_tiles(w, h):
    """Rectangles that cover the frame: columns of widths 1, 7, 13, 67, ... cut into rows of heights 3, 37, rest."""
    tiles, x, k = [], 0, 0
    while x < w:
        x1 = min(w, x + (1, 7, 13, 67)[k % 4])
        for y0, y1 in ((0, 3), (3, 40), (40, h)):
            tiles.append((x, y0, x1, y1))
        x, k = x1, k + 1
    return tiles


def resolve_expected(buf):
    """crh_ids_resolve in numpy float32: [..., 6, 2]."""
    ids, cnt, total = buf[..., 0:SLOTS], buf[..., SLOTS:2 * SLOTS], buf[..., TOTAL]
    order = np.argsort(-cnt.astype(np.int64), axis=-1, kind="stable")          # count descending; equal counts: the lower slot first
    ids, cnt = np.take_along_axis(ids, order, -1), np.take_along_axis(cnt, order, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = cnt.astype(np.float32) / total.astype(np.float32)[..., None]
    empty = (cnt == 0) | (total == 0)[..., None]
    out = np.empty(buf.shape[:-1] + (SLOTS, 2), np.float32)
    out[..., 0] = np.where(empty, np.float32(-1.0), ids.astype(np.float32))
    out[..., 1] = np.where(empty, np.float32(0.0), cov)
    return out
