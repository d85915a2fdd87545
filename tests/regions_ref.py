"""NumPy-only restatement of the map post-processing semantics (include/eae.h, "map post-processing"), written
to follow the text literally and slowly: a flood fill by an explicit stack for the regions, a double loop for the majority filter, the
six sieve rules with Python sets.  Every result is an integer array that the semantics define uniquely, so the GPU tests compare
with exact equality.  Also the map patterns the tests share."""
import numpy as np

N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def classified(labels, k):
    labels = np.asarray(labels)
    return (labels >= 0) & (labels < k)


def label_regions_ref(labels, k, connectivity=4):
    """regions int64 [H, W]: cells in raster order; an unvisited classified cell starts a region whose id is its own linear index (the
    smallest of the region: every cell with a smaller index was visited before), filled by an explicit stack.  -1: unclassified."""
    labels = np.asarray(labels)
    h, w = labels.shape
    ok = classified(labels, k).tolist()
    lab = labels.tolist()
    nbrs = N4 if connectivity == 4 else N8
    reg = [[-1] * w for _ in range(h)]
    for y0 in range(h):
        for x0 in range(w):
            if not ok[y0][x0] or reg[y0][x0] >= 0:
                continue
            rid, c = y0 * w + x0, lab[y0][x0]
            reg[y0][x0] = rid
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in nbrs:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and ok[yy][xx] and reg[yy][xx] < 0 and lab[yy][xx] == c:
                        reg[yy][xx] = rid
                        stack.append((yy, xx))
    return np.asarray(reg, dtype=np.int64).reshape(h, w)


def region_table_ref(labels, regions):
    """{"id", "cls", "area" [R], "bbox" [R, 4] = (y0, x0, y1, x1) inclusive}, int64, rows by ascending region id."""
    labels, regions = np.asarray(labels), np.asarray(regions)
    ids = np.unique(regions[regions >= 0])
    w = regions.shape[1]
    cls, area, bbox = [], [], []
    for r in ids.tolist():
        ys, xs = np.nonzero(regions == r)
        cls.append(labels[r // w, r % w])
        area.append(ys.size)
        bbox.append((ys.min(), xs.min(), ys.max(), xs.max()))
    return {"id": ids.astype(np.int64), "cls": np.asarray(cls, dtype=np.int64).reshape(-1),
            "area": np.asarray(area, dtype=np.int64).reshape(-1), "bbox": np.asarray(bbox, dtype=np.int64).reshape(-1, 4)}


def majority_ref(labels, k, radius=1, fill=False, passes=1):
    """The majority filter, cell by cell; each pass reads the whole output of the one before."""
    cur = np.asarray(labels).astype(np.int64)
    h, w = cur.shape
    for _ in range(passes):
        src, out = cur.tolist(), cur.copy()
        for y in range(h):
            for x in range(w):
                counts = {}
                for yy in range(max(0, y - radius), min(h, y + radius + 1)):
                    row = src[yy]
                    for xx in range(max(0, x - radius), min(w, x + radius + 1)):
                        c = row[xx]
                        if 0 <= c < k:
                            counts[c] = counts.get(c, 0) + 1
                centre = src[y][x]
                centre_ok = 0 <= centre < k
                if not counts or (not centre_ok and not fill):
                    continue                                      # stays as stored
                top = max(counts.values())
                tied = sorted(c for c, n in counts.items() if n == top)
                out[y, x] = centre if centre_ok and centre in tied else tied[0]
        cur = out
    return cur


def sieve_ref(labels, k, min_size, connectivity=4, passes=1):
    """(map, changed): the six rules of the sieve with Python sets; changed = the cells whose value changed in the last pass."""
    cur = np.asarray(labels).astype(np.int64)
    h, w = cur.shape
    changed = 0
    for _ in range(passes):
        reg = label_regions_ref(cur, k, connectivity)                                   # rule 1
        ids, counts = np.unique(reg[reg >= 0], return_counts=True)
        area = dict(zip(ids.tolist(), counts.tolist()))
        small = {r for r, a in area.items() if a < min_size}                            # rule 2
        cand = {r: set() for r in small}
        rl = reg.tolist()
        for y in range(h):
            for x in range(w):
                r = rl[y][x]
                if r not in small:                                                      # (-1 is in no set: rule 6)
                    continue
                for dy, dx in N4:                                                       # rule 3: edges, for both connectivities
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w:
                        q = rl[yy][xx]
                        if q >= 0 and q != r and q not in small:
                            cand[r].add(q)
        out = cur.copy()
        for r, qs in cand.items():
            if not qs:                                                                  # rule 5
                continue
            win = min(qs, key=lambda q: (-area[q], q))                                  # rule 4
            out[reg == r] = cur[win // w, win % w]
        changed = int((out != cur).sum())
        cur = out
    return cur, changed


# ---------------------------------------------------------------------------------------------------- patterns
def one_class(h, w):
    return np.full((h, w), 2, dtype=np.int64)


def checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return ((y + x) & 1).astype(np.int64)


def h_stripes(h, w):
    return np.repeat((np.arange(h) % 3)[:, None], w, 1).astype(np.int64)


def v_stripes(h, w):
    return np.repeat((np.arange(w) % 3)[None, :], h, 0).astype(np.int64)


def serpentine(h, w):
    """A 1-wide path of class 1 through a field of class 0: full rows at y = 0, 2, 4, ... joined at alternating ends."""
    m = np.zeros((h, w), dtype=np.int64)
    m[::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    """A 1-wide square spiral of class 1 in a field of class 0 (a gap of one cell between the turns)."""
    m = np.zeros((h, w), dtype=np.int64)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    y, x = 0, 0
    m[0, 0] = 1
    while True:
        moved = False
        for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            while top <= y + dy <= bottom and left <= x + dx <= right and m[y + dy, x + dx] == 0:
                ahead_y, ahead_x = y + 2 * dy, x + 2 * dx
                if 0 <= ahead_y < h and 0 <= ahead_x < w and m[ahead_y, ahead_x] == 1:
                    break                                         # keep one cell of gap to the previous turn
                y, x = y + dy, x + dx
                m[y, x] = 1
                moved = True
        if not moved:
            return m


def u_shapes(h, w):
    """Nested 'U's of alternating classes 1 and 2, 1 wide with a gap of class 0: the two arms of each rise through every tile row and
    join only in the bottom rows, inside another tile."""
    m = np.zeros((h, w), dtype=np.int64)
    for i, d in enumerate(range(0, min(h, w // 2), 2)):
        c = 1 + i % 2
        if w - 1 - d <= d:
            break
        m[:h - d, d] = c
        m[:h - d, w - 1 - d] = c
        m[h - 1 - d, d:w - d] = c
    return m


def diagonals(h, w):
    """1-wide diagonal lines of class 1 every 4 cells: singletons at 4-connectivity, lines at 8."""
    y, x = np.mgrid[:h, :w]
    return ((y - x) % 4 == 0).astype(np.int64)


def percolation(h, w, seed=0, p=0.59):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.int64)


def ten_class(h, w, seed=0, k=10):
    """Ten classes, 10 % of the cells -1, and a few cells K and K + 5 (which read as unclassified)."""
    rng = np.random.default_rng(seed + 77)
    m = rng.integers(0, k, (h, w)).astype(np.int64)
    m[rng.random((h, w)) < 0.1] = -1
    odd = rng.random((h, w)) < 0.02
    m[odd] = rng.choice([k, k + 5], int(odd.sum()))
    return m


def blobs(h, w, seed=0, k=10, block=3, noise=0.15):
    """A speckled land-cover-like map: block x block patches of one class with single-cell noise and 5 % unclassified cells."""
    rng = np.random.default_rng(seed + 5)
    coarse = rng.integers(0, k, (-(-h // block), -(-w // block)))
    m = np.repeat(np.repeat(coarse, block, 0), block, 1)[:h, :w].astype(np.int64)
    n = rng.random((h, w)) < noise
    m[n] = rng.integers(0, k, int(n.sum()))
    m[rng.random((h, w)) < 0.05] = -1
    return m
