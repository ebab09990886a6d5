"""The cluster queries' rules K1-K10 (include/simlod_hip.h, "cluster queries") one sample at a time in plain Python floats and integers: all
pairs, no grid and no union-find — rule C2 for every pair, a breadth-first search over the core graph, the border rule by an explicit minimum
over (d2, index) —, the restatement of cluster_rules.hpp's small functions, and the named inputs the io tier, the rules tier and the GPU tier
share.  Each input is small and each is a place where a kernel can go wrong; `case` says which."""
import math
from collections import deque

import numpy as np

import compare_ref as cr
from simlod_amd import abi

NOISE = 0xFFFFFFFF
MISS = 0xFFFFFFFF
SIZE_BINS = 33
NOISE_COLOR = 0xFF123456
TABLE = ((np.arange(256, dtype=np.uint64) * 0x01010101 + 0x00A0B0C0) & 0xFFFFFFFF).astype(np.uint32)


# ---- cluster_rules.hpp, restated ---------------------------------------------------------------------------------------------------------------
def params_acceptable(radius, min_neighbours, min_cluster_size, reserved=0):
    r = cr.f32(radius) if not math.isnan(radius) else radius
    return math.isfinite(r) and r >= 0.0 and min_neighbours >= 1 and min_cluster_size >= 1 and reserved == 0


def is_core(within, min_neighbours):
    return within >= min_neighbours


def size_bin(size):
    """floor(log2(size)) by counting the halvings (size >= 1; 0 for 0)."""
    b = 0
    while size > 1:
        size //= 2
        b += 1
    return b


def colour_index(cluster):
    return cluster % 256


def params(radius, min_neighbours=1, min_cluster_size=1, budget=0, wg=0, reserved=0, noise=NOISE_COLOR, table=TABLE):
    """One abi.cluster_params_dtype record, whatever it holds (the refused ones too)."""
    r = np.zeros(1, dtype=abi.cluster_params_dtype)
    with np.errstate(over="ignore"):
        r["radius"] = np.float32(radius)
    r["minNeighbours"], r["minClusterSize"], r["noiseColor"], r["maxCandidates"] = min_neighbours, min_cluster_size, noise, budget
    r["maxWorkgroups"], r["reserved"] = wg, reserved
    r["table"][0] = table
    return r


def record_acceptable(rec):
    r = np.asarray(rec).reshape(-1)[0]
    return params_acceptable(float(r["radius"]), int(r["minNeighbours"]), int(r["minClusterSize"]), int(r["reserved"]))


# ---- the rules, one sample at a time ----------------------------------------------------------------------------------------------------------
def cluster_exact(a, box_min, size, radius, min_neighbours, min_cluster_size, table=TABLE, noise_color=NOISE_COLOR, max_candidates=0, count_only=False,
                  return_links=False):
    """simlod_cluster_samples on `a` (abi.point_dtype) -> (records as abi.cluster_record_dtype, colours as uint32, the summary as an
    abi.cluster_summary_dtype record); records and colours are None for a count-only call and when the budget is exceeded.  return_links:
    the links between cores (i, j), i > j, as a fourth value."""
    mn = [float(np.float32(v)) for v in box_min]
    r = float(np.float32(radius))
    inv = cr.inv_of(r, float(np.float32(size)))
    rr = r * r
    p = cr._xyz(a)
    n = len(p)
    out = np.zeros((), dtype=abi.cluster_summary_dtype)
    valid = [i for i in range(n) if cr.is_valid(*p[i])]
    cells = {}
    for i in valid:
        c = cr.cell_of(p[i], mn, inv)
        cells[c] = cells.get(c, 0) + 1
    out["numInvalidA"] = out["numInvalidB"] = n - len(valid)
    out["numCells"], out["maxCellPopulation"] = len(cells), max(cells.values()) if cells else 0
    candidates = 0
    for i in valid:
        c = cr.cell_of(p[i], mn, inv)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if min(q) >= 0 and max(q) < cr.CELLS:
                        candidates += cells.get(q, 0)
    out["numCandidates"] = candidates
    if max_candidates != 0 and candidates > max_candidates:
        out["error"] = abi.CLUSTER_ERR_BUDGET
    if count_only or int(out["error"]) != 0:
        return (None, None, out, None) if return_links else (None, None, out)
    # rule K3: every pair once (d2 is symmetric bit for bit), a sample with itself (d2 = 0 <= rr)
    near = [[] for _ in range(n)]                                           # per sample the (d2, j) of the others that pass
    for x in range(len(valid)):
        i = valid[x]
        pi = p[i]
        ni = near[i]
        for y in range(x + 1, len(valid)):
            j = valid[y]
            d2 = cr.d2_of(p[j], pi)
            if d2 <= rr:
                ni.append((d2, j))
                near[j].append((d2, i))
    within = [0] * n
    for i in valid:
        within[i] = len(near[i]) + 1
    core = [False] * n
    for i in valid:
        core[i] = is_core(within[i], min_neighbours)
    # rule K4: breadth-first over the cores, from the lowest index up — the first core of a component to be met is its root
    root = [MISS] * n
    links = []
    for s in range(n):
        if not core[s] or root[s] != MISS:
            continue
        root[s] = s
        queue = deque([s])
        while queue:
            i = queue.popleft()
            for _, j in near[i]:
                if core[j] and root[j] == MISS:
                    root[j] = s
                    queue.append(j)
    if return_links:
        links = [(i, j) for i in range(n) if core[i] for _, j in near[i] if core[j] and j < i]
    # rule K5
    for i in valid:
        if core[i]:
            continue
        best = None
        for d2, j in near[i]:
            if core[j] and (best is None or (d2, j) < best):
                best = (d2, j)
        if best is not None:
            root[i] = root[best[1]]
    size_of = {}
    for i in range(n):
        if root[i] != MISS:
            size_of[root[i]] = size_of.get(root[i], 0) + 1                  # rule K6
    number = {}
    for s in sorted(size_of):                                               # rule K8
        if size_of[s] >= min_cluster_size:                                  # rule K7
            number[s] = len(number)
    rec = np.zeros(n, dtype=abi.cluster_record_dtype)
    colours = np.zeros(n, np.uint32)
    hist = [0] * SIZE_BINS
    n_core = n_border = n_noise = 0
    for i in range(n):
        s = root[i]
        if s == MISS:
            rec[i] = (NOISE, MISS, 0, within[i])
        else:
            rec[i] = (number.get(s, NOISE), s, size_of[s], within[i])
        if s in number:
            colours[i] = int(table[colour_index(number[s])])
            if core[i]:
                n_core += 1
            else:
                n_border += 1
        else:
            colours[i] = noise_color
            n_noise += 1
    largest, largest_number = 0, 0
    for s, k in number.items():
        hist[size_bin(size_of[s])] += 1
        if size_of[s] > largest or (size_of[s] == largest and k < largest_number):
            largest, largest_number = size_of[s], k
    out["numClusters"], out["numDissolved"] = len(number), len(size_of) - len(number)
    out["numCore"], out["numBorder"], out["numNoise"], out["numWithin"] = n_core, n_border, n_noise, sum(within)
    out["largestSize"], out["largestCluster"], out["sizeHist"] = largest, largest_number, hist
    return (rec, colours, out, links) if return_links else (rec, colours, out)


# ---- the named inputs: name -> (a, box_min, box_max, radius, min_neighbours, min_cluster_size) ---------------------------------------------------
def _shuffled(xyz, rs, lowest_at=None):
    """The positions in a random order; lowest_at: the position (row of xyz) that gets index 0."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    order = rs.permutation(len(xyz))                                        # order[index] = row
    if lowest_at is not None:
        k = int(np.flatnonzero(order == lowest_at)[0])
        order[0], order[k] = order[k], order[0]
    return cr.points(xyz[order])


def _line(n, step, origin=(0.0, 1.0, 1.0), axis=0):
    xyz = np.tile(np.asarray(origin, np.float64), (n, 1))
    xyz[:, axis] += np.arange(n) * step
    return xyz


def blob_centres():
    g = np.array([[8.0, 8.0, 8.0], [24.0, 8.0, 8.0], [8.0, 24.0, 8.0], [24.0, 24.0, 8.0], [8.0, 8.0, 24.0], [24.0, 8.0, 24.0], [8.0, 24.0, 24.0],
                  [24.0, 24.0, 24.0], [16.0, 16.0, 16.0], [16.0, 4.0, 16.0], [4.0, 16.0, 16.0], [16.0, 16.0, 28.0]])
    return g, np.linspace(0.4, 1.5, 12)


def case(name):
    rs = np.random.RandomState(29)
    unit = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    if name == "chain":                     # 3 000 samples on a line, exactly r apart (0.25 steps are exact: d2 == rr passes), 3 000 cells, twelve
        n = 3000                            # workgroups; index 0 sits in the middle: long chains of unions, and the root is still the minimum
        return _shuffled(_line(n, 0.25), rs, lowest_at=n // 2), (0.0, 0.0, 0.0), (1024.0, 1024.0, 1024.0), 0.25, 1, 1
    if name in ("gap_apart", "gap_touch"):  # two parallel chains: the next fp32 above r apart they stay two, exactly r apart they are one
        gap = float(np.nextafter(np.float32(0.25), np.float32(1.0))) if name == "gap_apart" else 0.25
        one = _line(200, 0.25, (0.0, 0.0, 1.0), axis=1)
        two = _line(200, 0.25, (gap, 0.0, 1.0), axis=1)
        return _shuffled(np.concatenate([one, two]), rs), (0.0, 0.0, 0.0), (64.0, 64.0, 64.0), 0.25, 1, 1
    if name in ("bridge", "bridge_tie"):    # minNeighbours 4: two dense groups and ONE sparse sample within r of one sample of each: a border
        left = [[1.0 - 0.125 * k, 1.0, 1.0] for k in range(6)]                  # sample; the groups stay two; it goes to the lower (d2, index)
        if name == "bridge":                # 0.4375 from the left group, 0.5 (== r) from the right one
            mid, right = [1.4375, 1.0, 1.0], [[1.9375 + 0.125 * k, 1.0, 1.0] for k in range(6)]
        else:                               # 0.5 from both: the index decides, and the right group's sample has the lower one
            mid, right = [1.5, 1.0, 1.0], [[2.0 + 0.125 * k, 1.0, 1.0] for k in range(6)]
        return cr.points(np.array(right + [mid] + left)), *unit, 0.5, 4, 1
    if name == "singletons":                # minNeighbours 1: about 2 000 isolated samples (clusters of size 1) mixed with 500 pairs, and
        g = np.arange(14) * 1.0 + 0.5       # minClusterSize 2: the numbering crosses the spans of the scan, the singles are dissolved
        at = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rs.permutation(14 ** 3)[:2500]]
        return _shuffled(np.concatenate([at, at[:500] + np.array([0.125, 0.0, 0.0])]), rs), (0.0, 0.0, 0.0), (16.0, 16.0, 16.0), 0.25, 1, 2
    if name == "duplicates":                # radius 0: coincident samples only — triples, pairs and singles; minNeighbours 2 makes the singles noise
        base = rs.rand(80, 3) * 4.0
        return _shuffled(np.concatenate([base, base[:40], base[:10]]), rs), *unit, 0.0, 2, 1
    if name == "hot_cell":                  # 600 samples in one cell and within r of each other: every pair is linked, one root takes it all
        h = cr.h_of(0.25, 4.0)
        return cr.points(5 * h + 0.05 + rs.rand(600, 3) * 0.14), *unit, 0.25, 1, 1
    if name == "cell_faces":                # samples at min + k*h and their ulp neighbours with a partner r away beyond the face; samples on the
        r = np.float32(0.3)                 # box's corners and edges and outside it, where the cell index clamps
        h = cr.h_of(float(r), 4.0)
        xs = []
        for k in (1, 2, 5, 9):
            v = np.float32(k * h)
            xs += [float(cr._ulp(v, False)), float(v), float(cr._ulp(v, True))]
        pts = [[x, 1.0, 1.0] for x in xs] + [[1.0, x, 2.0] for x in xs] + [[2.0, 1.0, x] for x in xs]
        far = []
        for q in pts:
            for k in range(3):
                for sgn in (-1.0, 1.0):
                    t = list(q)
                    t[k] = float(np.float32(t[k] + sgn * float(r)))
                    far.append(t)
        edge = [[0.0, 0.0, 0.0], [4.0, 4.0, 4.0], [4.0, 0.0, 2.0], [0.0, 4.0, 0.0], [-0.2, 0.1, 0.1], [-0.25, 0.1, 0.1], [4.3, 4.1, 3.9], [4.2, 4.2, 4.2],
                [5.0, 5.0, 5.0], [5.25, 5.0, 5.0], [-3.0, 2.0, 2.0], [-3.0, 2.25, 2.0], [2.0, 2.0, 9.0], [0.0, 0.0, 0.25]]
        return _shuffled(np.array(pts + far + edge), rs), *unit, float(r), 2, 1
    if name == "all_27":                    # ONE core in the middle of a cell, a sample in each of the 26 cells around it: minNeighbours 27
        h = cr.h_of(0.5, 4.0)
        c = (np.array([3.0, 3.0, 3.0]) + 0.5) * h
        off = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3) * 0.55 * h
        return _shuffled(c + off, rs), *unit, 0.5, 27, 1
    if name == "invalid":                   # NaN and both infinities spread through the array, a box off the origin
        mn, mx = (100.0, -50.0, 7.0), (104.0, -46.0, 11.0)
        a = cr.points(np.array(mn) + rs.rand(300, 3) * 4.0)
        for k, v in enumerate([np.nan, np.inf, -np.inf] * 8):
            a["xyz"[k % 3]][k * 12 + 1] = v
        a["x"][7], a["y"][8] = 1e30, -1e30
        return a, mn, mx, 0.6, 3, 2
    if name in ("blobs", "blobs_part"):     # 20 000 samples: twelve Gaussian blobs of different densities and uniform noise; blobs_part: the
        g, sigma = blob_centres()           # 1 500 of them nearest to the densest blob's centre, for the quadratic reference
        xyz = np.concatenate([g[k] + rs.randn(1500, 3) * sigma[k] for k in range(12)] + [rs.rand(2000, 3) * 32.0])
        a = _shuffled(xyz, rs)
        if name == "blobs_part":
            d = (a["x"].astype(np.float64) - g[0][0]) ** 2 + (a["y"].astype(np.float64) - g[0][1]) ** 2 + (a["z"].astype(np.float64) - g[0][2]) ** 2
            a = a[np.sort(np.argsort(d, kind="stable")[:1500])]
        return a, (0.0, 0.0, 0.0), (32.0, 32.0, 32.0), 0.2, 6, 10
    raise KeyError(name)


CASES = ["chain", "gap_apart", "gap_touch", "bridge", "bridge_tie", "singletons", "duplicates", "hot_cell", "cell_faces", "all_27", "invalid", "blobs"]
# the reference is quadratic: blobs is checked against it on blobs_part
EXACT_CASES = [c if c != "blobs" else "blobs_part" for c in CASES]


def case_record(name, **kw):
    """The abi.cluster_params_dtype record the case runs with."""
    _, _, _, radius, min_neighbours, min_cluster_size = case(name)
    return params(radius, min_neighbours, min_cluster_size, **kw)


def exact(name):
    """cluster_exact on the case (with its links)."""
    a, mn, mx, radius, min_neighbours, min_cluster_size = case(name)
    size = float((np.asarray(mx, np.float32) - np.asarray(mn, np.float32)).max())
    return cluster_exact(a, mn, size, radius, min_neighbours, min_cluster_size, return_links=True)
