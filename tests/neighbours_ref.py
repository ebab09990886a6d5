"""Shared by the neighbour-query tests: the seeded query sets, the brute force over an input array (which never went through an octree), an
exhaustive top-k over an export's samples without any culling, the lattice of exact ties, and the conditions that keep a comparison from
passing on nothing."""
import numpy as np

import cases
from simlod_amd import abi
from simlod_amd.octree_io import Spheres

N_QUERIES = 128
NONE = abi.EXPORT_NONE
K = 8                                   # the k at which the conditions below are stated


def is_big(box):
    return float(max(box)) > 2.0


def extent(pts):
    """The largest extent of the points' bounding box."""
    return float(max(float(pts[a].max()) - float(pts[a].min()) for a in "xyz"))


def radii(pts, box):
    """(wide, thin) radius of a case: fractions of the largest extent of the points' bounding box."""
    ext = extent(pts)
    return (0.004 * ext, 0.002 * ext) if is_big(box) else (0.064 * ext, 0.008 * ext)


def _chosen(pts, n=N_QUERIES):
    return np.sort(np.random.RandomState(42).choice(len(pts), n, replace=False))


def wide(pts, box):
    """128 input points (seed 42, sorted by index) at the wide radius: nearly every query has more than 8 points within it."""
    return Spheres.from_points(pts[_chosen(pts)], radii(pts, box)[0])


def thin(pts, box):
    """The same points, each moved by a uniform offset in [-r, r]^3 (seed 43), at the thin radius r: some queries find nothing, most of
    the others fewer than 8."""
    p = pts[_chosen(pts)]
    r = radii(pts, box)[1]
    c = np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float64) + (np.random.RandomState(43).rand(len(p), 3) * 2.0 - 1.0) * r
    return Spheres(c, r)


def query_sets(pts, box):
    return {"wide": wide(pts, box), "thin": thin(pts, box)}


def shift_spheres(spheres, offset):
    """The queries moved by `offset` as cases.shift_points moves points: float32(center + offset)."""
    s = spheres.record().copy()
    s["center"] = s["center"] + np.asarray(offset, dtype=np.float32)
    return Spheres.from_records(s)


def sample_d2(rec, i, x, y, z):
    """Rule 2 for query i of `rec` against float64 coordinate arrays -> (d2, passes)."""
    c, r = rec["center"][i].astype(np.float64), np.float64(rec["radius"][i])
    with np.errstate(invalid="ignore", over="ignore"):
        px, py, pz = x - c[0], y - c[1], z - c[2]
        d2 = (px * px + py * py) + pz * pz
        return d2, d2 <= r * r


def brute(spheres, pts, k):
    """The rule-2 arithmetic over raw points, query by query -> (the k smallest passing d2 ascending, padded with inf: (n, k); how many pass).
    The queries must be valid."""
    rec = spheres.record()
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    best, within = np.full((len(rec), k), np.inf), np.zeros(len(rec), np.int64)
    for i in range(len(rec)):
        d2, ok = sample_d2(rec, i, x, y, z)
        within[i] = int(ok.sum())
        d = np.sort(d2[ok])[:k]
        best[i, :len(d)] = d
    return best, within


def assert_found_are_brute(nb, within, spheres, pts, k, what=""):
    """The d2 lists are bit-equal to the k smallest brute-force d2 over `pts` (the same arithmetic), `within` equals the brute force, every
    found sample's 16 bytes are those of an input point at that d2, and the places behind min(k, within) are miss records."""
    rec = spheres.record()
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    keys = pts.view(np.uint64).reshape(-1, 2)
    best, bw = np.full((len(rec), k), np.inf), np.zeros(len(rec), np.int64)
    for i in range(len(rec)):
        d2, ok = sample_d2(rec, i, x, y, z)
        at = np.nonzero(ok)[0]
        bw[i] = len(at)
        d = np.sort(d2[at])[:k]
        best[i, :len(d)] = d
        assert int(within[i]) == bw[i] and np.array_equal(nb["d2"][i].view(np.uint64), best[i].view(np.uint64)), \
            f"{what}: query {i}: within {int(within[i])} / d2 {nb['d2'][i]}, the brute force has {bw[i]} / {best[i]}"
        for j in range(len(d)):
            same = at[d2[at] == d[j]]
            s = np.ascontiguousarray(nb["sample"][i, j:j + 1]).view(np.uint64).reshape(2)
            assert ((keys[same, 0] == s[0]) & (keys[same, 1] == s[1])).any(), f"{what}: query {i} place {j}: the sample is not an input point at that d2"
    assert_misses_behind(nb, bw, k, what)
    return best, bw


def assert_misses_behind(nb, within, k, what=""):
    behind = np.arange(k)[None, :] >= np.minimum(np.asarray(within, np.int64), k)[:, None]
    m = nb[behind]
    assert np.isposinf(m["d2"]).all() and (m["node"] == NONE).all() and (m["ordinal"] == NONE).all() and not np.ascontiguousarray(m["sample"]).view(np.uint8).any(), \
        f"{what}: a place behind min(k, within) is not the miss record"
    f = nb[~behind]
    assert np.isfinite(f["d2"]).all() and (f["node"] != NONE).all(), f"{what}: a miss record before min(k, within)"


def assert_found_index_export(nb, export, what=""):
    """export.samples[export.nodes[node].firstSample + ordinal] == record.sample for every found record."""
    f = nb[nb["node"] != NONE]
    assert (f["node"] < export.num_nodes).all() and (f["ordinal"] < export.nodes["numSamples"][f["node"]]).all(), f"{what}: a record outside its node"
    idx = export.nodes["firstSample"][f["node"]].astype(np.int64) + f["ordinal"]
    assert export.samples[idx].tobytes() == np.ascontiguousarray(f["sample"]).tobytes(), f"{what}: a record's sample is not the export's"


def exhaustive(export, spheres, k):
    """The result by an exhaustive search over ALL samples of the export's selected nodes, with no culling at all: per query the first k of
    the passing samples in the order (d2, node, ordinal) -> ((n, k) records, within)."""
    rec = spheres.record()
    tb, smp = export.nodes, export.samples
    x, y, z = (smp[a].astype(np.float64) for a in "xyz")
    node = np.repeat(np.arange(len(tb)), tb["numSamples"].astype(np.int64))
    ordinal = np.arange(len(smp)) - tb["firstSample"].astype(np.int64)[node]
    out = np.zeros((len(rec), k), dtype=abi.neighbour_dtype)
    out["d2"], out["node"], out["ordinal"] = np.inf, NONE, NONE
    within = np.zeros(len(rec), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(rec["center"]).all(1) & np.isfinite(rec["radius"]) & (rec["radius"] >= 0)
    for i in np.nonzero(valid)[0]:
        d2, ok = sample_d2(rec, i, x, y, z)
        at = np.nonzero(ok)[0]                                 # (samples are in (node, ordinal) order: a stable sort by d2 gives the total order)
        within[i] = len(at)
        at = at[np.argsort(d2[at], kind="stable")[:k]]
        m = len(at)
        out["d2"][i, :m], out["node"][i, :m], out["ordinal"][i, :m], out["sample"][i, :m] = d2[at], node[at], ordinal[at], smp[at]
    return out, within


def assert_thin_not_vacuous(within, what, k=K):
    """At k = 8 at least 5 % of the thin queries find nothing and at least 25 % find between 1 and k - 1."""
    w = np.asarray(within)
    none, some = float((w == 0).mean()), float(((w >= 1) & (w < k)).mean())
    assert none >= 0.05 and some >= 0.25, f"{what}: {none:.3f} of the queries find nothing, {some:.3f} find 1..{k - 1}"
    return none, some


def assert_wide_not_vacuous(within, what, k=K):
    """At k = 8 at least 25 % of the wide queries have within > k: the selection drops something."""
    more = float((np.asarray(within) > k).mean())
    assert more >= 0.25, f"{what}: only {more:.3f} of the queries have more than {k} within"
    return more


def assert_not_vacuous(key, within, what, k=K):
    return assert_thin_not_vacuous(within, what, k) if key == "thin" else assert_wide_not_vacuous(within, what, k)


# ---- the lattice of exact ties ---------------------------------------------------------------------------------------------------------
LATTICE_N = 64
LATTICE_BATCH = 65_536
LATTICE_K = 4


def lattice():
    """64^3 points at (i/64, j/64, k/64) in the unit box, coloured by their index -> (points, box)."""
    n = LATTICE_N
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    pts = np.zeros(n ** 3, dtype=abi.point_dtype)
    pts["x"], pts["y"], pts["z"] = i.reshape(-1) / n, j.reshape(-1) / n, k.reshape(-1) / n
    pts["color"] = np.arange(n ** 3, dtype=np.uint32)
    return pts, (1.0, 1.0, 1.0)


def lattice_queries(n=N_QUERIES, seed=44):
    """128 queries at interior lattice points of the plane x = 32/64 (the root's mid-plane), radius exactly 1/64: the point itself at d2 = 0
    and its six axis neighbours at d2 = 2^-12 exactly, the two along x in other level-1 nodes than the four in the plane's own."""
    rs = np.random.RandomState(seed)
    jk = rs.choice((LATTICE_N - 2) ** 2, n, replace=False)
    j, k = 1 + jk // (LATTICE_N - 2), 1 + jk % (LATTICE_N - 2)
    c = np.stack([np.full(n, LATTICE_N // 2), j, k], axis=1) / LATTICE_N
    return Spheres(c, 1.0 / LATTICE_N)


def assert_lattice_ties(nb, within, export, spheres, what=""):
    """Every query has within == 7 and itself at place 0; in at least 100 queries the samples at the fourth place's d2 belong to more than
    one node and the records are the smallest (node, ordinal) among them."""
    rec = spheres.record()
    assert (np.asarray(within) == 7).all(), f"{what}: within {np.unique(within)}"
    assert (nb["d2"][:, 0] == 0).all() and (nb["d2"][:, 1:LATTICE_K] == 2.0 ** -12).all(), what
    tb, smp = export.nodes, export.samples
    x, y, z = (smp[a].astype(np.float64) for a in "xyz")
    node = np.repeat(np.arange(len(tb)), tb["numSamples"].astype(np.int64))
    ordinal = np.arange(len(smp)) - tb["firstSample"].astype(np.int64)[node]
    spread = 0
    for i in range(len(rec)):
        d2, ok = sample_d2(rec, i, x, y, z)
        at = np.nonzero(ok & (d2 == nb["d2"][i, LATTICE_K - 1]))[0]
        assert len(at) == 6, (what, i, len(at))
        spread += len(np.unique(node[at])) > 1
        assert nb["node"][i, 1:LATTICE_K].tolist() == node[at[:LATTICE_K - 1]].tolist() and nb["ordinal"][i, 1:LATTICE_K].tolist() == ordinal[at[:LATTICE_K - 1]].tolist(), (what, i)
    assert spread >= 100, f"{what}: only {spread} queries have their ties in more than one node"


# ---- degenerate queries and rule 3 at its edge -------------------------------------------------------------------------------------------
def invalid_variants(good_record):
    """One good query spoiled in every way rule 1 names: NaN, +inf and -inf in each of the four floats, and two negative radii."""
    bad = []
    for f in range(4):
        for v in (np.nan, np.inf, -np.inf):
            r = good_record.copy()
            if f < 3:
                r["center"][0, f] = v
            else:
                r["radius"] = v
            bad.append(r)
    for v in (-0.5, -1e-30):
        r = good_record.copy()
        r["radius"] = v
        bad.append(r)
    return bad


def degenerate_batch(good, box, extra=()):
    """good[:8] | the invalid variants | valid oddities | good[8:] -> (Spheres, slice of the invalid ones, index of the first oddity).
    The oddities: `extra` records (e.g. radius 0 on duplicated points), a centre far outside the box with a small radius (no pair), a centre
    outside the box whose radius reaches in, a radius that covers the whole box."""
    g = good.record()
    b = np.asarray(box, dtype=np.float64)
    bad = invalid_variants(g[:1])
    odd = list(extra) + [Spheres([10.0 * b], 0.01 * b.max()).record(), Spheres([[-0.5 * b.max(), 0.5 * b[1], 0.5 * b[2]]], 0.6 * b.max()).record(),
                         Spheres([0.5 * b], 2.0 * b.max()).record()]
    rec = np.concatenate([g[:8]] + bad + odd + [g[8:]])
    return Spheres.from_records(rec), slice(8, 8 + len(bad)), 8 + len(bad)


def edge_queries(box, radius=0.5):
    """Rule 3 at its edge, for a box at the origin: [on the root cube's widened low x face minus the radius (pairs), one ulp further out (none),
    diagonally off the low x/y corner: within the radius of the cube on each axis, yet g2 > rr (none)].  The radius must make the face a float32."""
    size = np.float64(max(box))
    e = np.ldexp(size, -abi.MAX_DEPTH)
    face = np.float32(-(e + np.float64(np.float32(radius))))
    assert np.float64(face) == (0.0 - e) - np.float64(np.float32(radius)), "the face is not a float32: choose another radius"
    y, z = 0.5 * box[1], 0.5 * box[2]
    off = np.float32(-(e + 0.8 * radius))
    return Spheres([[float(face), y, z], [float(np.nextafter(face, np.float32(-np.inf))), y, z], [float(off), float(off), z]], radius)
