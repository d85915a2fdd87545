"""NumPy-only restatement of the superpixel semantics (include/eae.h, "superpixels"), written from the text and
not from the kernel: the quantiser, the initialisation, one iteration as a loop over the nine neighbour cells with Python-exact
int64 arithmetic, the rounded means, and the way from clusters to zones (one sieve pass, connected regions, dense ids) through
tests/regions_ref.py with a number of classes no label reaches.  Every result is an integer array that the semantics define
uniquely, so the GPU tests compare with exact equality.  Also the synthetic parcel scene the tests share."""
import numpy as np

from regions_ref import label_regions_ref, sieve_ref

U_ONE = 65535
ANY_LABEL = 2 ** 62                # "k" for regions_ref: every non-negative label is a class


def quantise_ref(scene, divisor):
    """u int64 [C, H, W] = rint(65535 * min(max(v / d, 0), 1)) in float64, NaN -> 0 (the comparisons are false for a NaN)."""
    scene = np.asarray(scene)
    c = scene.shape[0]
    d = np.broadcast_to(np.asarray(divisor, dtype=np.float32).reshape(-1), (c,)).astype(np.float64).reshape(c, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = scene.astype(np.float64) / d
        clamped = np.where(p > 0, np.where(p < 1, p, 1.0), 0.0)
    return np.rint(U_ONE * clamped).astype(np.int64)


def grid_ref(h, w, step):
    return -(-h // step), -(-w // step)


def weight_ref(compactness):
    return int(np.rint((np.float64(U_ONE) * np.float64(compactness)) ** 2))


def sums_ref(u, labels, n_cl):
    """sums int64 [n_cl, C + 3] = (count, sum y, sum x, sum u_c) over the pixels with label k."""
    c, h, w = u.shape
    y, x = np.mgrid[:h, :w]
    keep = labels >= 0
    k = labels[keep]
    cols = [np.ones(k.size, dtype=np.int64), y[keep], x[keep]] + [u[b][keep] for b in range(c)]
    # bincount adds in float64: exact here, every partial sum is an integer below 2^31 * 65535 < 2^53
    return np.stack([np.rint(np.bincount(k, weights=col, minlength=n_cl)).astype(np.int64) for col in cols], axis=1)


def centres_ref(sums):
    """centres int32: column 0 the count, every other column (2 sum + n) // (2 n); an empty cluster is all zeros."""
    n = sums[:, :1]
    safe = np.maximum(n, 1)
    means = np.where(n > 0, (2 * sums[:, 1:] + n) // (2 * safe), 0)
    return np.concatenate([n, means], axis=1).astype(np.int32)


def init_ref(u, step, mask=None):
    """labels int64 [H, W] of iteration 0: the home cluster, -1 for a masked pixel."""
    _, h, w = u.shape
    _, n_w = grid_ref(h, w, step)
    y, x = np.mgrid[:h, :w]
    labels = (y // step) * n_w + x // step
    if mask is not None:
        labels = np.where(np.asarray(mask) != 0, -1, labels)
    return labels.astype(np.int64)


def assign_ref(u, centres, step, weight, mask=None):
    """labels int64 [H, W] of an iteration t >= 1: over the nine neighbour cells in ascending cluster id, the smallest
    D = S^2 sum_c (u_c - mu_c)^2 + M ((y - cy)^2 + (x - cx)^2); a strict comparison keeps the lowest id on a tie."""
    c, h, w = u.shape
    n_h, n_w = grid_ref(h, w, step)
    cen = centres.astype(np.int64)
    y, x = np.mgrid[:h, :w]
    hi, hj = np.mgrid[:n_h, :n_w]                                  # the home cells; a candidate is the same for all pixels of one

    def pixels(a):                                                 # a per-cell array at pixel resolution
        return np.repeat(np.repeat(a, step, 0), step, 1)[:h, :w]

    best = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
    labels = np.full((h, w), -1, dtype=np.int64)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            i, j = hi + di, hj + dj
            inside = (i >= 0) & (i < n_h) & (j >= 0) & (j < n_w)
            kc = np.where(inside, i * n_w + j, 0)
            okc = inside & (cen[kc, 0] > 0)
            k, ok = pixels(kc), pixels(okc)
            colour = np.zeros((h, w), dtype=np.int64)
            for b in range(c):
                colour += (u[b] - pixels(cen[kc, 3 + b])) ** 2
            # (no candidate: nothing is evaluated -- its centre may lie anywhere)
            dy, dx = y - pixels(np.where(okc, cen[kc, 1], 0)), x - pixels(np.where(okc, cen[kc, 2], 0))
            dy, dx = np.where(ok, dy, 0), np.where(ok, dx, 0)
            d = step * step * colour + weight * (dy ** 2 + dx ** 2)
            assert (d >= 0).all()                                  # no overflow (the bound of DESIGN.md section 35)
            take = ok & (d < best)
            best = np.where(take, d, best)
            labels = np.where(take, k, labels)
    if mask is not None:
        labels = np.where(np.asarray(mask) != 0, -1, labels)
    return labels


def slic_ref(scene, divisor, step, weight, iterations, mask=None, history=False):
    """(labels, sums, centres) after ``iterations`` steps; history=True: the list of those triples after iteration 0, 1, ..."""
    u = quantise_ref(scene, divisor)
    _, h, w = u.shape
    n_h, n_w = grid_ref(h, w, step)
    labels = init_ref(u, step, mask)
    sums = sums_ref(u, labels, n_h * n_w)
    centres = centres_ref(sums)
    out = [(labels, sums, centres)]
    for _ in range(iterations):
        labels = assign_ref(u, centres, step, weight, mask)
        sums = sums_ref(u, labels, n_h * n_w)
        centres = centres_ref(sums)
        out.append((labels, sums, centres))
    return out if history else out[-1]


def default_min_size(step):
    return max(1, step * step // 4)


def zones_ref(labels, min_size, connectivity=4):
    """(zones int32 [H, W], Z): one sieve pass over the regions of equal label, the connected regions of the sieved labels, and dense
    ids in ascending order of a region's smallest linear index (which is the region's id)."""
    sieved, _ = sieve_ref(labels, ANY_LABEL, min_size, connectivity, passes=1)
    regions = label_regions_ref(sieved, ANY_LABEL, connectivity)
    ids = np.unique(regions[regions >= 0])
    zones = np.where(regions >= 0, np.searchsorted(ids, regions), -1).astype(np.int32)
    return zones, int(ids.size)


def slic_scene_ref(scene, divisor, step, compactness, iterations, mask=None, min_size=None, connectivity=4):
    """(zones, Z, labels, centres) of the whole pipeline."""
    labels, _, centres = slic_ref(scene, divisor, step, weight_ref(compactness), iterations, mask)
    zones, z = zones_ref(labels, default_min_size(step) if min_size is None else min_size, connectivity)
    return zones, z, labels, centres


def boundaries_ref(zones, connectivity=4):
    zones = np.asarray(zones)
    h, w = zones.shape
    out = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            nb = [(y, x + 1), (y + 1, x)] + ([(y + 1, x + 1), (y + 1, x - 1)] if connectivity == 8 else [])
            out[y, x] = any(0 <= yy < h and 0 <= xx < w and zones[yy, xx] != zones[y, x] for yy, xx in nb)
    return out


# the hand-worked case of tests/test_slic_reference.py (step 3, divisor 255, M = 1000)
HAND_SCENE = np.array([[[0, 0, 0, 10, 10, 10],
                        [0, 0, 10, 10, 10, 10],
                        [0, 0, 0, 10, 10, 10],
                        [20, 20, 20, 20, 20, 0]]], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- the parcel scene
def parcel_scene(h=96, w=128, parcels=12, bands=3, noise=6, seed=0):
    """(scene uint8 [bands, H, W], truth int64 [H, W]): Voronoi parcels of constant colour +- ``noise``."""
    rng = np.random.default_rng(seed)
    sites = np.stack([rng.integers(0, h, parcels), rng.integers(0, w, parcels)], axis=1)
    colours = rng.integers(30, 226, (parcels, bands))
    y, x = np.mgrid[:h, :w]
    d = (y[None] - sites[:, 0, None, None]) ** 2 + (x[None] - sites[:, 1, None, None]) ** 2
    truth = d.argmin(0).astype(np.int64)
    scene = colours[truth].transpose(2, 0, 1) + rng.integers(-noise, noise + 1, (bands, h, w))
    return np.clip(scene, 0, 255).astype(np.uint8), truth


def purity(zones, truth):
    """The share of the zoned pixels that carry the majority truth label of their zone."""
    keep = zones >= 0
    z, t = zones[keep].astype(np.int64), truth[keep]
    table = np.zeros((int(z.max()) + 1, int(t.max()) + 1), dtype=np.int64)
    np.add.at(table, (z, t), 1)
    return table.max(1).sum() / keep.sum()


def grid_zones(h, w, step):
    y, x = np.mgrid[:h, :w]
    return ((y // step) * (-(-w // step)) + x // step).astype(np.int64)
