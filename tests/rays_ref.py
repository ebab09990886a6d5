"""Shared by the ray-query tests: the seeded ray sets, the brute force over an input array (which never went through an octree), an
exhaustive search over an export's samples without any culling, and the conditions that keep a comparison from passing on nothing."""
import numpy as np

import cases
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Rays

N_RAYS = 128
SEED = 42
NONE = abi.EXPORT_NONE


def is_big(box):
    return float(max(box)) > 2.0


def _eye(box, offset=(0.0, 0.0, 0.0)):
    """The eye of cases._cam (cases.camera_pose 'bird')."""
    return np.array([1.8 * box[0], -1.2 * box[1], 1.4 * max(box)], dtype=np.float64) + np.asarray(offset, dtype=np.float64)


def vertical(pts, box, radius, n=N_RAYS, seed=SEED, offset=(0.0, 0.0, 0.0)):
    """Straight down over random positions of the box's footprint, from 10 above the box to 10 below it."""
    rs = np.random.RandomState(seed)
    o = np.asarray(offset, dtype=np.float64)
    xy = rs.rand(n, 2) * np.asarray(box[:2], dtype=np.float64) + o[:2]
    return Rays.vertical(xy, o[2] + box[2] + 10.0, radius, o[2] - 10.0)


def vertical_over_points(pts, box, radius, n=N_RAYS, seed=SEED):
    """The same over the footprint of the POINTS (the hotspot case fills one level-3 cell of its box)."""
    rs = np.random.RandomState(seed)
    lo = np.array([pts["x"].min(), pts["y"].min()], dtype=np.float64)
    hi = np.array([pts["x"].max(), pts["y"].max()], dtype=np.float64)
    return Rays.vertical(lo + rs.rand(n, 2) * (hi - lo), float(pts["z"].max()) + 0.1 * max(box), radius, float(pts["z"].min()) - 0.1 * max(box))


def cones(pts, box, spread, n=N_RAYS, seed=SEED, offset=(0.0, 0.0, 0.0), terrain_seed=3):
    """Cones of radius 0 and the given spread from the cases' camera eye, unit directions, to twice the distance of their targets: random
    ground positions of the synthetic terrain (big boxes), random positions in the points' bounding box (unit boxes)."""
    rs = np.random.RandomState(seed)
    o = np.asarray(offset, dtype=np.float64)
    if is_big(box):
        xy = rs.rand(n, 2) * np.asarray(box[:2], dtype=np.float64)
        h = synthetic._height(xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32), np.random.RandomState(terrain_seed + 1), np.asarray(box, dtype=np.float64))
        tgt = np.concatenate([xy, h.astype(np.float64)[:, None]], axis=1) + o
    else:
        lo = np.array([pts[a].min() for a in "xyz"], dtype=np.float64)
        hi = np.array([pts[a].max() for a in "xyz"], dtype=np.float64)
        tgt = lo + rs.rand(n, 3) * (hi - lo)
    eye = _eye(box, offset)
    d = tgt - eye
    dist = np.linalg.norm(d, axis=1)
    return Rays(np.broadcast_to(eye, d.shape), d / dist[:, None], 0.0, 2.0 * dist, 0.0, spread)


def random_rays(pts, box, radius, n=N_RAYS, seed=SEED):
    """Random origins in the points' bounding box, random directions of the unit cube (not normalised: t is in units of |dir|), tMax 2."""
    rs = np.random.RandomState(seed)
    lo = np.array([pts[a].min() for a in "xyz"], dtype=np.float64)
    hi = np.array([pts[a].max() for a in "xyz"], dtype=np.float64)
    org = lo + rs.rand(n, 3) * (hi - lo)
    d = (rs.rand(n, 3) - 0.5) * max(box)
    return Rays(org, d, 0.0, 2.0, radius, 0.0)


# name -> (builder, needs misses too, a cone set)
def ray_sets(name, pts, box):
    """The ray sets of a case of tests/cases.py at the origin: {set name: (Rays, needs_misses, is_cone_set)}.  needs_misses: the brute force
    gives the set a hit share well below 0.95, so both outcomes must be represented."""
    if name == "terrain_4x100k":
        return {"vertical r0.5": (vertical(pts, box, 0.5), True, False), "vertical r0.25": (vertical(pts, box, 0.25), True, False),
                "vertical r1": (vertical(pts, box, 1.0), False, False), "cones s0.0005": (cones(pts, box, 0.0005), True, True),
                "cones s0.002": (cones(pts, box, 0.002), False, True)}
    if name == "hotspot_150k":      # 150 000 points in a cell of 1/8: the same sets over the points' own extent, radii scaled by 1/8
        return {"vertical r0.0002": (vertical_over_points(pts, box, 0.0002), True, False), "random r0.0025": (random_rays(pts, box, 0.0025), False, False),
                "cones s0.0005": (cones(pts, box, 0.0005), False, True)}
    return {"random r0.005": (random_rays(pts, box, 0.005), True, False), "random r0.02": (random_rays(pts, box, 0.02), False, False),
            "vertical r0.003": (vertical_over_points(pts, box, 0.003), False, False), "cones s0.002": (cones(pts, box, 0.002), False, True)}


def covered_pixels(transform, width, height, pts):
    """The pixels some point of `pts` projects into, as the rasteriser maps them ((ndc * 0.5 + 0.5) * size), in raster order: (n, 2)."""
    m = np.asarray(transform, dtype=np.float64).reshape(4, 4)
    c = np.stack([pts["x"], pts["y"], pts["z"], np.ones(len(pts), np.float32)], axis=1).astype(np.float64) @ m.T
    pix = np.floor((c[:, :2] / c[:, 3:4] * 0.5 + 0.5) * [width, height]).astype(np.int64)
    ok = (c[:, 3] > 0) & (pix >= 0).all(1) & (pix[:, 0] < width) & (pix[:, 1] < height)
    flat = np.unique(pix[ok, 1] * width + pix[ok, 0])
    return np.stack([flat % width, flat // width], axis=1)


def shift_rays(rays, offset):
    """The rays moved by `offset` as cases.shift_points moves points: float32(origin + offset)."""
    r = rays.record().copy()
    r["origin"] = r["origin"] + np.asarray(offset, dtype=np.float32)
    return Rays.from_records(r)


def _fields(rec):
    o, d = rec["origin"].astype(np.float64), rec["dir"].astype(np.float64)
    return o, d, rec["tMin"].astype(np.float64), rec["tMax"].astype(np.float64), rec["radius"].astype(np.float64), rec["spread"].astype(np.float64)


def sample_test(rec, i, x, y, z):
    """Rule 2 for ray i of `rec` against float64 coordinate arrays -> (t, passes)."""
    o, d, tmin, tmax, rad, spr = _fields(rec[i:i + 1])
    dx, dy, dz = d[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        px, py, pz = x - o[0, 0], y - o[0, 1], z - o[0, 2]
        dd = (dx * dx + dy * dy) + dz * dz
        t = ((dx * px + dy * py) + dz * pz) / dd
        qx, qy, qz = px - t * dx, py - t * dy, pz - t * dz
        s2 = (qx * qx + qy * qy) + qz * qz
        rr = rad[0] + spr[0] * t
        return t, (t >= tmin[0]) & (t <= tmax[0]) & (s2 <= rr * rr)


def brute(rays, pts):
    """The rule-2 arithmetic over raw points, ray by ray -> (t of the nearest passing point or inf, how many pass, how many attain that t).
    The rays must be valid."""
    rec = rays.record()
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    tmin, npass, nbest = np.full(len(rec), np.inf), np.zeros(len(rec), np.int64), np.zeros(len(rec), np.int64)
    for i in range(len(rec)):
        t, ok = sample_test(rec, i, x, y, z)
        npass[i] = int(ok.sum())
        if npass[i]:
            tmin[i] = t[ok].min()
            nbest[i] = int((ok & (t == tmin[i])).sum())
    return tmin, npass, nbest


def assert_hits_are_brute(hits, rays, pts, what=""):
    """Every hit's t is the brute-force minimum over `pts` (bit-equal: the same arithmetic), its 16 bytes are those of a point that attains
    it, and hit / miss agree for every ray."""
    rec = rays.record()
    tmin, npass, nbest = brute(rays, pts)
    hit = hits["node"] != NONE
    assert np.array_equal(hit, npass > 0), f"{what}: hit / miss differ from the brute force at rays {np.nonzero(hit != (npass > 0))[0][:8]}"
    assert np.array_equal(hits["t"].view(np.uint64), tmin.view(np.uint64)), f"{what}: t differs from the brute-force minimum"
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    keys = pts.view(np.uint64).reshape(-1, 2)
    for i in np.nonzero(hit)[0]:
        t, ok = sample_test(rec, i, x, y, z)
        best = ok & (t == tmin[i])
        s = np.ascontiguousarray(hits["sample"][i:i + 1]).view(np.uint64).reshape(2)
        assert ((keys[best, 0] == s[0]) & (keys[best, 1] == s[1])).any(), f"{what}: ray {i}'s sample is not an input point at the minimum"
    return tmin, npass, nbest


def exhaustive(export, rays):
    """The hits by an exhaustive search over ALL samples of the export's selected nodes, with no culling at all: per ray the minimum of
    (t, node, ordinal) over the samples that pass rule 2."""
    rec = rays.record()
    tb, smp = export.nodes, export.samples
    x, y, z = (smp[a].astype(np.float64) for a in "xyz")
    node = np.repeat(np.arange(len(tb)), tb["numSamples"].astype(np.int64))
    ordinal = np.arange(len(smp)) - tb["firstSample"].astype(np.int64)[node]
    hits = np.zeros(len(rec), dtype=abi.ray_hit_dtype)
    hits["t"], hits["node"], hits["ordinal"] = np.inf, NONE, NONE
    for i in range(len(rec)):
        t, ok = sample_test(rec, i, x, y, z)
        if not ok.any():
            continue
        k = np.nonzero(ok & (t == t[ok].min()))[0][0]          # (samples are in (node, ordinal) order)
        hits["t"][i], hits["node"][i], hits["ordinal"][i], hits["sample"][i] = t[k], node[k], ordinal[k], smp[k]
    return hits


def assert_not_vacuous(hits, needs_misses, what, passing=None, cone=False):
    """At least a quarter of the rays hit; where the set is meant to have both outcomes, at least 5 % miss; in a cone set at least half of
    the hits had more than one passing sample to choose from."""
    hit = hits["node"] != NONE
    share = float(hit.mean())
    assert share >= 0.25, f"{what}: only {share:.2f} of the rays hit"
    if needs_misses:
        assert share <= 0.95, f"{what}: {share:.2f} of the rays hit, too few misses"
    if cone:
        assert passing is not None and float((passing[hit] > 1).mean()) >= 0.5, f"{what}: the arg-min has nothing to choose from"
    return share


def assert_hits_index_export(hits, export, what=""):
    """export.samples[export.nodes[node].firstSample + ordinal] == hit.sample for every hit; a miss is the miss record."""
    hit = hits["node"] != NONE
    h = hits[hit]
    assert (h["node"] < export.num_nodes).all() and (h["ordinal"] < export.nodes["numSamples"][h["node"]]).all(), f"{what}: a hit outside its node"
    idx = export.nodes["firstSample"][h["node"]].astype(np.int64) + h["ordinal"]
    assert export.samples[idx].tobytes() == np.ascontiguousarray(h["sample"]).tobytes(), f"{what}: a hit's sample is not the export's"
    m = hits[~hit]
    assert np.isposinf(m["t"]).all() and (m["ordinal"] == NONE).all() and not np.ascontiguousarray(m["sample"]).view(np.uint8).any(), f"{what}: a miss is not the miss record"
