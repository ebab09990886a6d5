"""Shared by tests/test_gpu_builder_states.py and tests/test_builder_states_io.py: the inputs of the builder states, the query sets one
battery asks of every state, the guards that keep a comparison from passing on nothing, the precondition helpers, and `collapse`, which
turns a full export into the octree a builder without free node slots leaves behind (leaves of more than 50 chunks).  The battery holds a
region, a footprint, rays, spheres, a view with its budget and delta, a profile, two paints, pack / unpack, a lasso on the view's screen,
summaries of the region, the lasso and the whole box, and the inverse of the region, the footprint and the lasso as a query, a summary and a
paint each.  Everything here is numpy on host arrays: nothing depends on the code under test."""
from collections import namedtuple

import numpy as np

import cases
import footprint_ref as fr
import inverse_ref as ir
import lasso_ref as lr
import neighbours_ref as nr
import oracle
import pack_ref as kr
import paint_ref as pf
import profile_ref as pr
import rays_ref as yr
import region_ref as rr
import summary_ref as zr
import view_ref as vr
from export_ref import export_host
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Footprint, Lasso, OctreeExport, Paint, Profile, Rays, Region, Spheres, _box_of, classify_footprint, classify_lasso, classify_nodes

State = namedtuple("State", "dev u pts box")            # the device object, its uniforms, the points the octree holds NOW, the box
ROW = 50                                                 # chunk addresses a row of the builder's chunk table holds (LEAF_ROW_SLOTS)
OVER = abi.MAX_POINTS_PER_NODE                           # a leaf above this has a split pending
N_QUERIES, K = 64, 16
H_POINTS = 600_000                                       # the smallest multiple of 300 000 terrain points at which state H exists (test_builder_states_io)
ERR_SPILLED, ERR_NODES = 0x2, 0x8                        # SIMLOD_ERR_SPILLED_OVERFLOW, SIMLOD_ERR_NODES_EXHAUSTED (include/simlod_hip.h)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def a_input():
    """State A: 600 000 uniform points in four batches; with room for nine nodes the root splits once and its eight leaves keep growing.
    -> (points, box, batches)"""
    pts, box = synthetic.uniform_cube(600_000, seed=5)
    return pts, box, [pts[i:i + 150_000] for i in range(0, len(pts), 150_000)]


def b_input():
    """State B: A's points and 200 000 more of the same stream -> (all 800 000 points, box, the 200 000 in two batches)"""
    pts, box = synthetic.uniform_cube(800_000, seed=5)
    assert pts[:600_000].tobytes() == a_input()[0].tobytes()
    return pts, box, [pts[600_000:700_000], pts[700_000:]]


def e_input():
    """State E: the terrain of the case terrain_4x100k, six batches of 100 000 -> (points, box, batches)"""
    pts, box = synthetic.terrain(600_000, seed=3, box=(600.0, 400.0, 40.0), tile=50.0)
    return pts, box, [pts[i:i + 100_000] for i in range(0, len(pts), 100_000)]


def f_input():
    """State F: four uniform batches of 500 000 -> (points, box, batches)"""
    pts, box = synthetic.uniform_cube(2_000_000, seed=17)
    return pts, box, [pts[i:i + 500_000] for i in range(0, len(pts), 500_000)]


def c_input(n):
    """State C: the slab of test_scarce_scratch_defers_splits_without_losing_a_point (a uniform cube with z * 0.02: leaves fill up together) with
    n points, in batches of 500 000 -> (points, box, batches)"""
    pts, box = synthetic.uniform_cube(n, seed=99)
    pts["z"] *= np.float32(0.02)
    return pts, box, [pts[i:i + 500_000] for i in range(0, len(pts), 500_000)]


def oracle_build(box, batches, persistent=1 << 30, capacity=None, mask=None):
    """The port oracle's octree of `batches`, one launch per batch -> (HostOctree, uniforms, allocatedBytes_persistent after each batch taken)"""
    u = cases.uniforms_for(box, np.eye(4, dtype=np.float32), persistent=capacity or persistent)
    ho = oracle.HostOctree("port", persistent_bytes=persistent, ring_slots=abi.BATCH_STREAM_SIZE)
    if mask is not None:
        ho.set_trunk_mask(*mask)
    ho.reset(u)
    after = []
    for b in batches:
        ho.upload(b)
        ho.construct(u)
        assert ho.last_error() == 0
        after.append(int(ho.stats["allocatedBytes_persistent"][0]))
    return ho, u, after


def export_of(ho, u):
    t, s = export_host(ho.nodes, int(ho.stats["numNodes"][0]))
    return OctreeExport(t, s, u["boxMin"], u["boxMax"])


def f_capacity(box, batches):
    """State F's persistentBufferCapacity: the guard takes a batch while allocator offset + 200 MB < capacity, so a capacity midway between
    the oracle's allocator offsets after one and after two batches (+ 200 MB) lets the second batch in and refuses the third."""
    _, _, after = oracle_build(box, batches[:2])
    assert after[0] < after[1]
    return (after[0] + after[1]) // 2 + 200_000_000, after


# ---- collapse ----------------------------------------------------------------------------------------------------------------------------------
def collapse(ex, level=1):
    """The full export `ex` with everything below `level` folded into its ancestor at `level`: those entries become leaves that hold the
    points of every leaf under them (in table order), the entries above keep their voxels.  What a builder leaves that could not split
    below `level`, up to the order of a leaf's points."""
    t, s = ex.nodes, ex.samples
    n = len(t)
    lv = t["level"].astype(np.int64)
    anc = np.arange(n)
    par = t["parent"].astype(np.int64)
    for i in range(1, n):                                   # (breadth-first: a parent comes before its children)
        if lv[i] > level:
            anc[i] = anc[par[i]]
    keep = int((lv <= level).sum())
    assert (lv[:keep] <= level).all()
    out = t[:keep].copy()
    leaf_src = (t["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    ns = t["numSamples"].astype(np.int64)
    first = t["firstSample"].astype(np.int64)
    parts, counts = [], np.zeros(keep, np.int64)
    for i in range(keep):
        if lv[i] < level and not leaf_src[i]:
            idx = [i]                                        # an inner node above the level: its voxels
        else:
            idx = [j for j in np.nonzero(anc == i)[0] if leaf_src[j]]
        for j in idx:
            parts.append(s[first[j]: first[j] + ns[j]])
            counts[i] += ns[j]
    at = lv[:keep] == level
    out["childMask"][at], out["firstChild"][at] = 0, abi.EXPORT_NONE
    out["flags"] = np.where(out["childMask"] == 0, abi.EXPORT_FLAG_LEAF, 0) | abi.EXPORT_FLAG_SELECTED
    out["numSamples"] = counts
    out["firstSample"] = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    samples = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)
    return OctreeExport(out, samples, ex.box_min, ex.box_max)


# ---- per-node comparisons ----------------------------------------------------------------------------------------------------------------------
def per_node(ex, leaves):
    """The samples of the leaves (16 bytes each) or of the inner nodes (positions only: which point coloured a voxel depends on the launch),
    sorted within each node, with the node's key in front: equal arrays <=> equal multisets per node."""
    t = ex.nodes
    owner = np.repeat(np.arange(len(t)), t["numSamples"].astype(np.int64))
    pick = ((t["flags"][owner] & abi.EXPORT_FLAG_LEAF) != 0) == leaves
    w = ex.samples.view(np.uint32).reshape(-1, 4)[pick].astype(np.uint64)
    if not leaves:
        w[:, 3] = 0
    from util import node_keys
    key = node_keys(t)[owner[pick]]
    rows = np.concatenate([key[:, None], w], axis=1)
    return rows[np.lexsort([rows[:, c] for c in range(4, -1, -1)])]


def assert_same_per_node(got, want, what):
    assert got.nodes.tobytes() == want.nodes.tobytes(), f"{what}: the tables differ"
    for leaves in (True, False):
        assert np.array_equal(per_node(got, leaves), per_node(want, leaves)), f"{what}: the samples differ per node (leaves={leaves})"


# ---- preconditions -----------------------------------------------------------------------------------------------------------------------------
def overfull_leaves(table):
    """The leaf entries of an export's table that hold more than SIMLOD_MAX_POINTS_PER_NODE samples."""
    t = np.asarray(table)
    return np.nonzero(((t["flags"] & abi.EXPORT_FLAG_LEAF) != 0) & (t["numSamples"] > OVER))[0]


def assert_state_a(dbg, table):
    """Node array full: the error bit, nine nodes, eight leaves of more than 50 000 points (more chunks than a table row has slots)."""
    assert int(dbg) == ERR_NODES, f"Stats.dbg {int(dbg):#x}"
    assert len(table) == 9, f"{len(table)} nodes"
    over = overfull_leaves(table)
    assert len(over) == 8 and (table["level"][over] == 1).all(), f"{len(over)} over-full leaves"
    assert (table["numSamples"][over] > ROW * abi.POINTS_PER_CHUNK).all()


def assert_state_c(dbg, table):
    """Scarce scratch: the spill bit alone, at least one leaf with a pending split beside leaves that did split (an inner node below the root)."""
    assert int(dbg) == ERR_SPILLED, f"Stats.dbg {int(dbg):#x}"
    assert len(overfull_leaves(table)) >= 1, "no leaf with a pending split"
    assert int(((table["flags"] & abi.EXPORT_FLAG_LEAF) == 0).sum()) > 1, "no leaf split"
    return len(overfull_leaves(table))


def assert_stopped_short(stats, taken, pending, guard=False):
    """A launch sequence that left batches pending: `taken` ingested, `pending` of them still in the ring (the host knows how many it uploaded)."""
    assert int(stats["dbg"]) == 0 and int(stats["batchletIndex"]) == taken and pending > 0, (int(stats["dbg"]), int(stats["batchletIndex"]), pending)
    assert int(stats["memCapacityReached"]) == int(guard), f"memCapacityReached {int(stats['memCapacityReached'])}"


def assert_no_overfull(table):
    over = overfull_leaves(table)
    assert len(over) == 0, f"{len(over)} leaves above {OVER} points, the largest {int(np.asarray(table)['numSamples'][over].max())}"


def h_input(partition, n=H_POINTS):
    """State H: rank 0's share of an n-point terrain split over two ranks (partition: test_gpu_trunk._partition), in batches of 300 000
    -> (all points, box, the trunk mask, the rank's points, its batches)"""
    pts, box = synthetic.terrain(n, seed=4, box=(600.0, 400.0, 40.0))
    dest, mask = partition(pts, box, 2)
    mine = pts[dest == 0]
    return pts, box, tuple(int(m) for m in mask), mine, [mine[i:i + 300_000] for i in range(0, len(mine), 300_000)]


def points_in_nodes(table, pts, box):
    """How many of `pts` lie in the cube of each table entry (the builder's cell arithmetic: floor(2^level * p / size), fp32)."""
    size = np.float32(max(box))
    out = np.zeros(len(table), np.int64)
    for lv in np.unique(table["level"]):
        at = np.nonzero(table["level"] == lv)[0]
        c = [np.minimum((np.float32(2.0 ** int(lv)) * pts[a] / size).astype(np.int64), 2 ** int(lv) - 1) for a in "xyz"]
        key = (c[0] << 42) | (c[1] << 21) | c[2]
        keys, cnt = np.unique(key, return_counts=True)
        want = (table["X"][at].astype(np.int64) << 42) | (table["Y"][at].astype(np.int64) << 21) | table["Z"][at].astype(np.int64)
        pos = np.searchsorted(keys, want)
        hit = (pos < len(keys)) & (keys[np.minimum(pos, len(keys) - 1)] == want)
        out[at] = np.where(hit, cnt[np.minimum(pos, len(keys) - 1)], 0)
    return out


def assert_masked_rank(table, pts, mine, box, mask):
    """State H: a mask is set, and it forces something — at least one node of the rank's octree holds none of the rank's points although the
    whole input has points in its cube (it exists for the other rank's sake).  -> how many"""
    assert tuple(int(m) for m in mask) != (0, 0), "no trunk mask"
    forced = int(((points_in_nodes(table, mine, box) == 0) & (points_in_nodes(table, pts, box) > 0)).sum())
    assert forced >= 1, "every node holds points of the rank or of nobody: the mask forces nothing"
    return forced


# ---- the battery's queries and their guards ----------------------------------------------------------------------------------------------------
Queries = namedtuple("Queries", "region footprint rays spheres radius profile lasso foot_lasso z0 scale")
W, H = cases.W, cases.H


def screen_lasso(transform, pts):
    """lasso_ref's "half" — the left half of the screen — scaled onto the PICTURE of `pts` under the camera `transform` (row-major, as the
    uniforms store it): its right edge stands at the median pixel column of the points in front of the eye, the other three edges one extent
    of the picture (its 2 % .. 98 % quantiles) outside it.  So the lasso holds half the points in front of the eye wherever they lie in the
    box (a launch that stopped short, the hotspot's one cell), the nodes left of the median column can be copied whole, the nodes it crosses
    are filtered, and the nodes right of it are outside — where the octree has nodes small enough for either (Shape, below)."""
    m = np.asarray(transform, np.float64).reshape(4, 4)
    p = np.stack([pts[a].astype(np.float64) for a in "xyz"] + [np.ones(len(pts))], axis=1)
    wc = p @ m[3]
    front = wc > 0
    assert front.any(), "no point in front of the eye"
    u, v = (p[front] @ (0.5 * W * (m[0] + m[3]))) / wc[front], (p[front] @ (0.5 * H * (m[1] + m[3]))) / wc[front]
    lo, hi = np.array([np.quantile(u, 0.02), np.quantile(v, 0.02)]), np.array([np.quantile(u, 0.98), np.quantile(v, 0.98)])
    a, b = lo - (hi - lo), np.array([float(np.median(u)), hi[1] + (hi[1] - lo[1])])
    half = lr.pixels("half").astype(np.float64)                # (0, 0) .. (W / 2, H)
    return Lasso.from_pixels(m, W, H, a + half / np.array([W / 2, H]) * (b - a))


def bins_of(lo, ext):
    """test_gpu_inverse._bins for the heights the points span (z0 a tenth of the span above the lowest, 256 bins over 0.7 of it): samples
    below bin 0 and above bin 255 exist and are clamped -> (z0, scale) as float32"""
    return np.float32(float(lo) + 0.1 * float(ext)), np.float32(256.0 / (0.7 * float(ext)))


def queries(pts, box, transform=None):
    """One query of each kind for an octree that holds `pts` in `box`, made from the points alone (a launch that stopped short holds
    points in a part of its box only, the hotspot in one level-3 cell: every query is placed by the points' bounding box, `the cube` below is
    its larger xy extent — for a filled box the octree's cube): region_ref's oblique half-space through the middle of that box; a
    seven-pointed star around the xy middle of its lower-left quarter, radii 0.6 and 0.5 of the cube — the LINE through any of its
    edges passes the middle at 0.49, outside the quarter's corners at 0.3536, so rule F3 finds every edge far from the nodes over that
    quarter and they are copied whole, while the nodes its points cross are filtered; 64 rays, each through a chosen point from 0.3 extents
    away in a random direction, and 64 spheres at the same points, with the radius at which a sphere around a chosen point holds 32 points in
    the median (twice k = 16: the top-k drops something; a ray's cylinder of half that radius holds its own point and, in the median, more);
    a corridor of half-width 0.27 cubes along three vertices: from 0.1 cubes left of the box at a quarter of its y extent to the bend at 0.6
    of its x extent, and up to 0.9 of its y extent.  On a filled square that is (-0.1, 0.25), (0.6, 0.25), (0.6, 0.9): segment 0's rectangle holds
    the whole plan square of the lower-left quarter (x -0.1 .. 0.6, y -0.02 .. 0.52), so rule P3 copies the nodes over it as the star does, its rim
    and segment 1 filter their neighbours, and the two rectangles overlap over x 0.33 .. 0.6, y 0.25 .. 0.52, where the lower segment owns the
    samples.  The bend and the end go by the extent of EACH axis, so that on a strip of points (the first batches of a terrain, whose cube is the
    long side) both segments and their overlap still hold points; only the half-width is the cube's.  transform (the battery's view camera):
    screen_lasso on the points' picture under it, the footprint once more as a lasso (Lasso.from_footprint: it must select what the footprint
    selects), and the bins of the summaries over the heights the points span (bins_of)."""
    lo = np.array([float(pts[a].min()) for a in "xyz"])
    ext = np.array([float(pts[a].max()) for a in "xyz"]) - lo
    size = float(ext[:2].max())
    star = Footprint.from_xy(fr.star(lo[0] + 0.25 * size, lo[1] + 0.25 * size, 0.6 * size, 0.5 * size, 7))
    rs = np.random.RandomState(77)
    at = np.sort(rs.choice(len(pts), N_QUERIES, replace=False))
    c = np.stack([pts[a][at] for a in "xyz"], axis=1).astype(np.float64)
    xyz = np.stack([pts[a] for a in "xyz"], axis=1).astype(np.float64)
    d32 = np.array([np.partition(((xyz - q) ** 2).sum(1), 2 * K)[2 * K] for q in c])
    radius = float(np.sqrt(np.median(d32)))
    d = rs.randn(N_QUERIES, 3)
    d *= 0.3 * nr.extent(pts) / np.linalg.norm(d, axis=1)[:, None]
    rays = Rays(c - d, d, 0.0, 2.0, 0.5 * radius, 0.0)
    bend = (lo[0] + 0.6 * ext[0], lo[1] + 0.25 * ext[1])
    corridor = Profile.from_xy([(lo[0] - 0.1 * size, bend[1]), bend, (bend[0], lo[1] + 0.9 * ext[1])], 0.27 * size)
    lasso = None if transform is None else screen_lasso(transform, pts)
    return Queries(rr.region("oblique", ext, lo), star, rays, Spheres(c, radius), radius, corridor, lasso, Lasso.from_footprint(star), *bins_of(lo[2], ext[2]))


def assert_crop_not_vacuous(cnt, what, copies=True):
    """As the region and footprint modules guard theirs: some nodes copied whole, some filtered, and the filter drops something.
    copies=False: an octree on which the query CANNOT copy a node (state A's root and eight octants under a plane through the middle) — then
    none is, and every node with samples is filtered."""
    copied, filtered = int(cnt["numCopiedNodes"]), int(cnt["numFilteredNodes"])
    assert (copied > 0 if copies else copied == 0) and filtered > 0, f"{what}: {copied} copied / {filtered} filtered"
    assert 0 < int(cnt["numSamples"]) < int(cnt["numCandidates"]), f"{what}: {int(cnt['numSamples'])} of {int(cnt['numCandidates'])} candidates"


def assert_rays_not_vacuous(hits, passing, what):
    yr.assert_not_vacuous(hits, False, what)
    hit = hits["node"] != abi.EXPORT_NONE
    assert float((passing[hit] > 1).mean()) >= 0.5, f"{what}: the arg-min has nothing to choose from"


def assert_spheres_not_vacuous(within, what):
    nr.assert_wide_not_vacuous(within, what, K)


def view_uniforms(box, camera="closer"):
    """The uniforms of the battery's view on the host (the device's differ in the buffer capacities, which no view rule reads)."""
    return vr.uniforms_of(box, vr.transform_of(camera, box))


def coarser_budget(ladder):
    """A sample budget that bias 0 misses and a later bias fits: S(b) of the first b with 0 < S(b) < S(0) -> (budget, b)"""
    for b in range(1, len(ladder)):
        if all(s > ladder[b] for s in ladder[:b]) and 0 < ladder[b]:
            return ladder[b], b
    raise AssertionError(f"no coarser cut with samples in the ladder {ladder}")


def assert_view_not_vacuous(cnt, what):
    assert int(cnt["error"]) == 0 and 0 < int(cnt["numSelected"]) and 0 < int(cnt["numSamples"]), f"{what}: {cnt}"


def assert_delta_not_vacuous(delta, what, adds=True):
    """The bias-2 cut against the bias-0 cut: the finer cut adds nodes and sends their samples.  adds=False: an octree whose two cuts are the
    same nodes (state A: the eight leaves or nothing) — everything is kept and nothing is sent."""
    s = delta.entries["state"]
    if adds:
        assert delta.num_samples > 0 and int((s == abi.DELTA_ADDED).sum()) > 0, f"{what}: nothing added"
    else:
        assert delta.num_samples == 0 and int((s == abi.DELTA_KEPT).sum()) > 0 and int((s == abi.DELTA_ADDED).sum()) == 0, f"{what}: not all kept"


# ---- the mirrors of one battery, guarded and held against brute force ------------------------------------------------------------------------
# What the guards can ask of an octree, stated per state (a flag that is False asserts the OPPOSITE, so each is a fact about the octree and not
# a check left out): `camera` of the view; whether the region / the footprint copies a node whole; whether the bias-0 cut adds nodes to the
# bias-2 cut; whether the view's ladder has a coarser rung with samples (without one a budget of S(0) - 1 chooses the first EMPTY cut); whether
# the profile copies a node whole; whether the screen lasso copies a node whole (an octree of a root and eight octants seen from inside has none
# in front of the eye whole, and under `closer` the octants of a small octree are wider than half the picture); whether the region / the
# footprint / the lasso leaves a node WITH samples outside — the nodes its inverse copies whole, as the nodes a selection copies are the ones its
# inverse lists at zero samples (rule I2); whether every leaf is longer than a chunk-table row — then every inverse result and every summary
# must hold samples from behind the row.
Shape = namedtuple("Shape", "camera region_copies footprint_copies delta_adds coarser profile_copies lasso_copies region_culls footprint_culls lasso_culls long_leaves",
                   defaults=("closer", True, True, True, True, True, True, True, True, True, False))
# a root and eight leaves of 75 chunks: the plane through the middle cuts all eight, the star leaves none outside, the eye is inside the box
NINE_NODES = Shape("inside", region_copies=False, delta_adds=False, lasso_copies=False, region_culls=False, footprint_culls=False, long_leaves=True)
ROOT_LEAF = Shape("closer", False, False, False, False, False, False, False, False, False)      # one node: filtered by everything, the only cut there is
SUMMARY_SUBSET, SUMMARY_SEED = 4096, 53                                 # samples summary_ref's per-sample Python loop takes of a larger selection
PAINT_SEED = 91                                                         # of the colours of the battery's ARRAY paint


def mirrors(full, pts, uv, what, shape=Shape(), pairs_all=False):
    """What the battery expects of an octree whose anchored full export is `full` and which holds `pts`, from the numpy mirrors alone: every
    answer guarded (above), the cuts equal to the brute-force filters of `pts`, the rays' t and the spheres' d2 bit-equal to the brute force
    over `pts`, the delta consistent in itself; the profile, the two paint calls and the packed export as profile_mirrors, paint_mirrors and
    pack_mirror (below) hold them, the lasso, the summaries and the inverses as lasso_mirrors, summary_mirrors and inverse_mirrors.  `uv`: the
    view's uniforms at bias 0, whose camera is the lasso's screen too.  pairs_all: rays and spheres with select "all" too."""
    import delta_ref
    mn, size = np.asarray(full.box_min, np.float64), np.asarray(full.box_max, np.float64) - np.asarray(full.box_min, np.float64)
    assert not mn.any()
    q = queries(pts, tuple(size), uv["transform"])
    m = {"q": q, "crop": {}, "rays": {}, "spheres": {}}
    for kind, region, foot in (("region", q.region, None), ("footprint", Region(), q.footprint)):
        for sel in ("cut", "all"):
            m["crop"][kind, sel] = full.crop(region, 20, sel, return_counts=True, footprint=foot)
        assert_crop_not_vacuous(m["crop"][kind, "cut"][1], f"{what} {kind}", shape.region_copies if kind == "region" else shape.footprint_copies)
    rr.assert_same_multiset(m["crop"]["region", "cut"][0].samples, pts[rr.brute_mask(q.region, pts)], f"{what} region")
    rr.assert_same_multiset(m["crop"]["footprint", "cut"][0].samples, pts[fr.contains_exact(q.footprint, pts)], f"{what} footprint")
    for sel in ("cut", "all") if pairs_all else ("cut",):
        hits, cnt, passing = full.cast(q.rays, 20, sel, return_counts=True, return_passing=True)
        nb, within, ncnt = full.neighbours(q.spheres, K, 20, sel, return_counts=True)
        m["rays"][sel], m["spheres"][sel] = (hits, cnt), (nb, within, ncnt)
        if sel == "cut":
            assert_rays_not_vacuous(hits, passing, f"{what} rays")
            assert_spheres_not_vacuous(within, f"{what} spheres")
            assert_hits_are_brute(hits, q.rays, pts, f"{what} rays")
            nr.assert_found_are_brute(nb, within, q.spheres, pts, K, f"{what} spheres")
    m["view"] = full.view(uv, return_counts=True)
    assert_view_not_vacuous(m["view"][1], f"{what} view")
    ladder = [int(v) for v in m["view"][1]["samplesAt"]]
    if shape.coarser:
        m["budget"], b = coarser_budget(ladder)
        m["coarser"] = full.view(uv, budget=m["budget"], return_counts=True)
        assert int(m["coarser"][1]["bias"]) == b > 0 and int(m["coarser"][1]["error"]) == 0 and 0 < int(m["coarser"][1]["numSamples"]) < ladder[0]
    else:
        assert all(s in (0, ladder[0]) for s in ladder), f"{what}: the ladder {ladder} has a coarser rung"
        m["budget"] = ladder[0] - 1
        m["coarser"] = full.view(uv, budget=m["budget"], return_counts=True)
        assert (int(m["coarser"][1]["error"]), int(m["coarser"][1]["numSamples"])) == (0, 0) and int(m["coarser"][1]["bias"]) > 0     # the empty cut fits
    m["held"] = full.view(uv, bias=2)
    m["delta"] = full.view_delta(uv, m["held"], tails=True)
    assert_delta_not_vacuous(m["delta"], f"{what} delta", shape.delta_adds)
    delta_ref.assert_delta_consistent(m["delta"], m["held"], m["view"][0])
    m["profile"] = profile_mirrors(full, q.profile, pts, what, shape.profile_copies)
    m["paint"] = paint_mirrors(full, q, tuple(size), m["crop"], what)
    m["pack"] = pack_mirror(full, what)
    # rule I1 over the points held and over every sample of the export (the voxels among them), once for all that follows
    gone = {kind: ir.passes_inverse(*sel3, pts) for kind, sel3 in selections(q).items()}
    gone_all = {kind: ir.passes_inverse(*sel3, full.samples) for kind, sel3 in selections(q).items()}
    m["lasso"] = lasso_mirrors(full, q, pts, ~gone["lasso"], m["crop"], what, shape)
    m["summary"] = summary_mirrors(full, q, pts, gone, gone_all, m["crop"], m["lasso"], what, shape)
    m["inverse"] = inverse_mirrors(full, q, pts, gone, gone_all, m["crop"], m["lasso"], m["summary"], tuple(size), what, shape)
    return m


def selections(q):
    """The battery's three selections, one per family of the inverse, as (region, footprint, lasso)"""
    return {"region": (q.region, None, None), "footprint": (Region(), q.footprint, None), "lasso": (Region(), None, q.lasso)}


def selection_classes(full, sel3):
    """The POSITIVE query's (outside, copied) per entry of the full export, the polygons' classes combined as rules F4 / L4 combine them."""
    region, fp, lasso = sel3
    outside, inside = classify_nodes(np.asarray(region.planes, np.float32).astype(np.float64), full.nodes, full.box_min, full.box_max)
    if fp is not None:
        near, corner = classify_footprint(fp, full.nodes, full.box_min, full.box_max)
        outside, inside = outside | (~near & ~corner), inside & ~near & corner
    if lasso is not None:
        behind, covered = classify_lasso(lasso, full.nodes, full.box_min, full.box_max)
        outside, inside = outside | behind, inside & covered
    return outside, inside


def behind_row(full, index):
    """How many of the samples full.samples[index] lie in a LEAF at an ordinal of ROW chunks or more: in a chunk that no row of the builder's
    chunk table names, which the read side reaches by `next` alone (from firstSample / numSamples and the chunk size)."""
    t = full.nodes
    first = t["firstSample"].astype(np.int64)
    index = np.asarray(index, np.int64)
    node = np.searchsorted(first, index, side="right") - 1             # (entries without samples share their successor's firstSample and come before it)
    assert ((index >= first[node]) & (index < first[node] + t["numSamples"][node].astype(np.int64))).all()
    leaf = (t["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    return int((leaf[node] & (index - first[node] >= ROW * abi.POINTS_PER_CHUNK)).sum())


def lasso_mirrors(full, q, pts, inside, crops, what, shape=Shape()):
    """OctreeExport.crop(lasso=) of the screen lasso at level 20 for "cut" and "all", and of the footprint's lasso for "cut"
    -> {"cut" / "all" / "footprint": (export, counts)}.  The screen lasso's cut is guarded as the crops are and is rule L1 decided exactly over
    `pts` (inside: lasso_ref.contains_exact's mask, through inverse_ref.passes_inverse); the footprint's lasso returns the footprint crop's samples (as a multiset: the two polygons' node rules need not copy the same nodes)."""
    m = {sel: full.crop(Region(), 20, sel, return_counts=True, lasso=q.lasso) for sel in ("cut", "all")}
    assert_crop_not_vacuous(m["cut"][1], f"{what} lasso", shape.lasso_copies)
    rr.assert_same_multiset(m["cut"][0].samples, pts[inside], f"{what} lasso")
    m["footprint"] = full.crop(Region(), 20, "cut", return_counts=True, lasso=q.foot_lasso)
    rr.assert_same_multiset(m["footprint"][0].samples, crops["footprint", "cut"][0].samples, f"{what}: the footprint as a lasso")
    return m


def summarize_whole(samples, box_min, size, z0, scale):
    """summary_ref's rules S1-S4 once more for FINITE samples, a whole selection at a time: the cells, the bins and their clamps in numpy
    float64 as summary_ref words them (one subtraction, one multiplication, truncation), sums and counts in uint64.  Written from summary_ref,
    sharing nothing with octree_io; assert_summary_is_exact holds it against the per-sample loop before it relies on it."""
    mn, inv = [float(np.float32(v)) for v in box_min], zr.inv_of(float(np.float32(size)))
    rec = np.zeros((), dtype=abi.summary_dtype)
    rec["numSamples"] = len(samples)
    c16 = []
    for k, a in enumerate("xyz"):
        v = samples[a]
        assert np.isfinite(v).all()
        rec["min"][k], rec["max"][k] = v.min(), v.max()
        t = (v.astype(np.float64) - mn[k]) * inv
        c = np.where(t >= 1048575.0, 1048575.0, np.where(t > 0.0, t, 0.0)).astype(np.uint64)
        rec["sum"][k] = c.sum(dtype=np.uint64)
        c16.append(c >> np.uint64(4))
    for j, (a, b) in enumerate(zr.MOMENTS):
        rec["sum2"][j] = (c16[a] * c16[b]).sum(dtype=np.uint64)
    t = (samples["z"].astype(np.float64) - float(np.float32(z0))) * float(np.float32(scale))
    rec["histZ"] = np.bincount(np.where(t >= 255.0, 255.0, np.where(t > 0.0, t, 0.0)).astype(np.int64), minlength=256)
    for k in range(4):
        rec["histC"][k] = np.bincount((samples["color"] >> np.uint32(8 * k)) & np.uint32(255), minlength=256)
    return rec


def _same_record(got, want, what):
    for f in abi.summary_dtype.names:                           # (the extent by value: the two zeros compare equal)
        same = np.array_equal(got[f], want[f]) if f in ("min", "max") else got[f].tobytes() == want[f].tobytes()
        assert same, f"{what}: {f} differs: {got[f]} != {want[f]}"


def assert_summary_is_exact(summary, selected, full, q, what):
    """A mirror's Summary against summary_ref over `selected`, the brute-force selection: every field of the record.  Up to SUMMARY_SUBSET
    samples summary_ref.summarize_exact (one sample at a time, in Python integers) gives the record itself.  More: the per-sample loop takes
    a fixed seeded subset of SUMMARY_SUBSET of them and holds summarize_whole, the same rules vectorised, on exactly that subset; the record of
    the WHOLE selection — count, extent, sums, moments, every bin of the five histograms — is then summarize_whole's."""
    n = len(selected)
    assert summary.num_samples == n > 0, f"{what}: the summary counts {summary.num_samples} samples, the brute force selects {n}"
    size = _box_of(full.box_min, full.box_max)[1]
    sub = selected if n <= SUMMARY_SUBSET else selected[np.sort(np.random.RandomState(SUMMARY_SEED).choice(n, SUMMARY_SUBSET, replace=False))]
    want = zr.summarize_exact(sub, full.box_min, size, q.z0, q.scale)
    _same_record(summarize_whole(sub, full.box_min, size, q.z0, q.scale), want, f"{what}: the vectorised rules against the per-sample loop on {len(sub)} samples")
    if n <= SUMMARY_SUBSET:
        assert summary.tobytes() == want.tobytes(), what
    _same_record(summary, summarize_whole(selected, full.box_min, size, q.z0, q.scale), what)


def summary_mirrors(full, q, pts, gone, gone_all, crops, lassos, what, shape=Shape()):
    """OctreeExport.summarize with the bins of q -> {(kind, sel): (Summary, counts, the table of the crop it summarises)} for the region ("cut" and "all"), the screen lasso and the
    whole box ("cut"; the box "all" too: the halves of rule I7 add up to it).  Each "cut" is held against summary_ref over the brute-force
    selection of `pts` (assert_summary_is_exact), the region's "all" over the brute-force selection of the export's samples.  A condition on the
    bins: the whole box fills more than half of them, and both end bins, where rule E3 clamps."""
    nobody = np.ones(len(pts), bool)
    m = {}
    for kind, region, lasso, sel, selected in (("region", q.region, None, "cut", pts[~gone["region"]]),
                                               ("region", q.region, None, "all", full.samples[~gone_all["region"]]),
                                               ("lasso", Region(), q.lasso, "cut", pts[~gone["lasso"]]),
                                               ("box", Region(), None, "cut", pts[nobody]), ("box", Region(), None, "all", full.samples)):
        table = crops["region", sel][0].nodes if kind == "region" else lassos[sel][0].nodes if kind == "lasso" else full.crop(Region(), 20, sel).nodes
        m[kind, sel] = full.summarize(region, 20, sel, z0=q.z0, scale=q.scale, return_counts=True, lasso=lasso) + (table,)
        assert len(table) == int(m[kind, sel][1]["numNodes"])
        assert_summary_is_exact(m[kind, sel][0], selected, full, q, f"{what} summary {kind} {sel}")
    hz = m["box", "cut"][0]["histZ"].reshape(-1)
    assert int((hz > 0).sum()) > 128 and hz[0] > 0 and hz[255] > 0, f"{what} summary: {int((hz > 0).sum())} bins filled, {int(hz[0])} / {int(hz[255])} samples in the end bins"
    if shape.long_leaves:                                       # (what contributes to a cut's summary: the leaves' samples the exact rule selects)
        in_leaf = np.repeat((full.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0, full.nodes["numSamples"].astype(np.int64))
        for kind, mask in (("region", ~gone_all["region"]), ("lasso", ~gone_all["lasso"]), ("box", True)):
            assert int((in_leaf & mask).sum()) == m[kind, "cut"][0].num_samples
            assert behind_row(full, np.nonzero(in_leaf & mask)[0]) > 0, f"{what} summary {kind}: no contributing sample lies behind a leaf's row"
    return m


InversePaint = namedtuple("InversePaint", "sel3 paint colors with_previous export counts previous")
SET_COLOR = 0x11223344


def inverse_mirrors(full, q, pts, gone, gone_all, crops, lassos, summaries, size, what, shape=Shape()):
    """OctreeExport.crop / summarize / paint with invert=True for the battery's three selections -> {"query": {(kind, sel): (export, counts)},
    "summary": {(kind, sel): (Summary, counts)}, "paint": [InversePaint x 3], "classes": {kind: (emptied, copied) nodes of the cut}}.
    Each cut is rule I1 decided exactly over `pts` (inverse_ref.passes_inverse) and, with the positive cut, holds `pts` exactly once; each
    "all" result is, sample for sample and in the export's order, what the same rule leaves of the export's samples (the voxels of filtered inner
    nodes among them).  The summaries, cut and all, are summary_ref's of those selections and add up with the positive query's to the whole
    box's (rules I6 / I7).  Guards, conditions on the
    selections: every inverse returns at least one sample and not every candidate; the nodes the positive query copies are listed at zero
    samples (Q_EMPTIED) and the nodes it leaves outside are copied whole — at least one of each among the cut's leaves, or none where the Shape
    says so; with long leaves every "all" result holds samples from behind a row.  The paints, each on top of the one before: a SET by the
    region's inverse WITHOUT `previous` (the path that stores without loading), a height ramp by the footprint's, an ARRAY of seeded colours by the
    lasso's; `previous` written back in reverse order, each in its query's order, gives `full`."""
    m = {"query": {}, "summary": {}, "paint": [], "classes": {}, "index": {}}
    leaf = (full.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    ns = full.nodes["numSamples"].astype(np.int64)
    in_leaf = np.repeat(leaf, ns)
    positive = {"region": crops["region", "cut"], "footprint": crops["footprint", "cut"], "lasso": lassos["cut"]}
    flags = {"region": (shape.region_copies, shape.region_culls), "footprint": (shape.footprint_copies, shape.footprint_culls), "lasso": (shape.lasso_copies, shape.lasso_culls)}
    for kind, sel3 in selections(q).items():
        region, fp, lasso = sel3
        outside, inside = selection_classes(full, sel3)
        cls = ir.class_map(outside, inside)
        for sel in ("cut", "all"):
            ex, cnt, index = full.crop(region, 20, sel, return_counts=True, footprint=fp, lasso=lasso, invert=True, return_index=True)
            m["query"][kind, sel], m["index"][kind, sel] = (ex, cnt), index
            assert 1 <= int(cnt["numSamples"]) <= int(cnt["numCandidates"]) - 1, f"{what} inverse {kind} {sel}: {int(cnt['numSamples'])} of {int(cnt['numCandidates'])} candidates"
            # rule I3: every node is listed, in the export's order; rule I2 per node
            chosen = (ns > 0) & (leaf if sel == "cut" else True)
            got = ex.nodes["numSamples"].astype(np.int64)
            assert len(got) == full.num_nodes and (got[chosen & (cls == ir.EMPTIED)] == 0).all() and (got[chosen & (cls == ir.COPIED)] == ns[chosen & (cls == ir.COPIED)]).all(), \
                f"{what} inverse {kind} {sel}: an emptied node keeps samples or a copied one loses some"
            assert int(cnt["numCopiedNodes"]) == int((chosen & (cls == ir.COPIED)).sum()) and int(cnt["numFilteredNodes"]) == int((chosen & (cls == ir.FILTERED)).sum())
            # rule I1 on every sample of the selected nodes: the result is exactly the samples that fail, in the export's order
            assert np.array_equal(index, np.nonzero(gone_all[kind] & (in_leaf if sel == "cut" else True))[0]), f"{what} inverse {kind} {sel}: not the samples the exact rule leaves"
            m["summary"][kind, sel] = full.summarize(region, 20, sel, footprint=fp, lasso=lasso, z0=q.z0, scale=q.scale, return_counts=True, invert=True)
            assert_summary_is_exact(m["summary"][kind, sel][0], full.samples[index] if sel == "all" else pts[gone[kind]], full, q, f"{what} inverse summary {kind} {sel}")
            if (kind, sel) in summaries:                        # (the footprint's halves: tests/test_builder_states_io.py)
                assert_halves_add_up(summaries[kind, sel][0], m["summary"][kind, sel][0], summaries["box", sel][0], f"{what} inverse summary {kind} {sel}")
            if shape.long_leaves and sel == "all":
                assert behind_row(full, index) > 0, f"{what} inverse {kind} all: no sample from behind a leaf's row"
        emptied, copied = int((leaf & (ns > 0) & (cls == ir.EMPTIED)).sum()), int((leaf & (ns > 0) & (cls == ir.COPIED)).sum())
        m["classes"][kind] = (emptied, copied)
        assert emptied == int(positive[kind][1]["numCopiedNodes"]), f"{what} inverse {kind}: {emptied} emptied leaves, the positive cut copies {int(positive[kind][1]['numCopiedNodes'])}"
        assert ((emptied > 0) == flags[kind][0]) and ((copied > 0) == flags[kind][1]), f"{what} inverse {kind}: {emptied} leaves emptied / {copied} copied whole, the shape says {flags[kind]}"
        inv = m["query"][kind, "cut"][0]
        rr.assert_same_multiset(inv.samples, pts[gone[kind]], f"{what} inverse {kind}")
        # (the positive cut is pts[~gone] as a multiset — mirrors and lasso_mirrors hold it against the same exact rules —: the two cuts partition `pts`)
        assert inv.num_samples + positive[kind][0].num_samples == len(pts), f"{what} inverse {kind}: the two halves do not hold the points once"
    state = full
    n = int(m["query"]["lasso", "all"][1]["numSamples"])
    colors = np.random.RandomState(PAINT_SEED + 1).randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for kind, paint, col, with_previous in (("region", Paint.set(SET_COLOR), None, False), ("footprint", pf.paints(size)["ramp"], None, True), ("lasso", Paint.array(), colors, True)):
        region, fp, lasso = selections(q)[kind]
        e, c, prev = state.paint(region, paint, footprint=fp, lasso=lasso, colors=col, return_previous=True, invert=True)
        assert c.tobytes() == m["query"][kind, "all"][1].tobytes() and len(prev) == int(c["numSamples"]), f"{what} inverse paint {kind}: not the inverse query's counts"
        assert (e.samples["color"] != state.samples["color"]).any(), f"{what} inverse paint {kind}: the call changes nothing"
        assert np.array_equal(prev, state.samples["color"][m["index"][kind, "all"]]), f"{what} inverse paint {kind}: previous is not in the inverse query's order"
        m["paint"].append(InversePaint(selections(q)[kind], paint, col, with_previous, e, c, prev))
        state = e
    back = state.samples["color"].copy()                        # the undo: an ARRAY paint writes previous[j] to sample j of the query's order (rule I8)
    for kind, call in reversed(list(zip(selections(q), m["paint"]))):
        back[m["index"][kind, "all"]] = call.previous
    assert np.array_equal(back, full.samples["color"]) and state.nodes.tobytes() == full.nodes.tobytes(), f"{what} inverse paint: the undo is not the octree before"
    return m


def assert_forced_empty_listed(full, inverse, pts, mine, box):
    """State H: at least one node the mask forces (assert_masked_rank) holds no sample before any query — the rank never put a point under it
    —, and every inverse table lists it where the export does, at zero samples: a node that reaches the classes of rule I2 empty.  -> how many"""
    t = full.nodes
    empty = (points_in_nodes(t, mine, box) == 0) & (points_in_nodes(t, pts, box) > 0) & (t["numSamples"] == 0)
    assert int(empty.sum()) >= 1, "every node the mask forces holds samples"
    for key, (ex, cnt) in inverse["query"].items():
        e = ex.nodes
        assert len(e) == len(t) and all(np.array_equal(e[f][empty], t[f][empty]) for f in ("level", "X", "Y", "Z")) and not e["numSamples"][empty].any(), f"inverse {key}: a forced empty node"
    return int(empty.sum())


def assert_halves_add_up(pos, inv, whole, what):
    """Rules I6 / I7 on summaries: a selection's and its inverse's count, sums and histograms add up to the whole box's, field by field."""
    assert pos.num_samples + inv.num_samples == whole.num_samples, f"{what}: {pos.num_samples} + {inv.num_samples} samples of {whole.num_samples}"
    for f in ("histC", "histZ", "sum", "sum2", "numNonFinite"):
        assert np.array_equal(pos[f] + inv[f], whole[f]), f"{what}: {f} of the two halves does not add up to the whole box's"


def words(a):
    """16-byte records as rows of four uint32 words"""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def sorted_rows(a):
    """The rows of a 2-D array in one fixed order (that of their bytes): equal results <=> equal multisets of rows"""
    a = np.ascontiguousarray(a)
    return np.sort(a.view(np.dtype((np.void, a.shape[1] * a.itemsize))).ravel())


def profile_mirrors(full, profile, pts, what, copies=True):
    """OctreeExport.profile at level 20 for "cut" and "all" -> {sel: (export, records, counts)}.  The cut is guarded as the crops are and held
    against rule P1 decided exactly over `pts`: its samples are the points in some segment, its (sample, record) pairs those of Profile.records on
    them, as multisets.  Conditions on the corridor, not measurements: it has samples in segment 0 and in segment 1, and the bend's overlap holds a
    point that lies in both rectangles and is recorded under the lower segment."""
    m = {sel: full.profile(profile, None, 20, sel, return_counts=True) for sel in ("cut", "all")}
    ex, rec, cnt = m["cut"]
    assert_crop_not_vacuous(cnt, f"{what} profile", copies)
    seg = pr.locate_exact(profile, pts)
    inside = pts[seg >= 0]
    rr.assert_same_multiset(ex.samples, inside, f"{what} profile")
    records = profile.records(inside)
    got = np.concatenate([words(ex.samples), words(rec)], axis=1)
    ref = np.concatenate([words(inside), words(records)], axis=1)
    assert np.array_equal(sorted_rows(got), sorted_rows(ref)), f"{what} profile: (sample, record) pairs differ from Profile.records on the points held"
    assert np.array_equal(records["segment"].astype(np.int64), seg[seg >= 0]), f"{what} profile: a record's segment is not the exact rule's"
    assert len(profile) == 3
    second = pr.locate_exact(Profile(profile.vertices[1:], profile.half_width, profile.axis_u, profile.axis_v, profile.axis_h), pts) >= 0
    assert (seg == 0).any() and (seg == 1).any() and ((seg == 0) & second).any(), \
        f"{what} profile: {int((seg == 0).sum())} / {int((seg == 1).sum())} points in segments 0 / 1, {int(((seg == 0) & second).sum())} in the overlap under segment 0"
    return m


PaintCall = namedtuple("PaintCall", "region footprint paint colors export counts previous")


def paint_mirrors(full, q, size, crops, what):
    """The battery's two paint calls on the host, the second on top of the first -> [PaintCall, PaintCall]: BLEND on (q.region, no footprint),
    then ARRAY with seeded random colours on (no planes, q.footprint); each with the export after it, its counts and `previous`.  Rule E0: a
    call's counts are the "all" crop's of the same region and footprint, so the crops' guards cover the paint.  The two `previous` arrays painted
    back in reverse order give `full` back."""
    blend = pf.paints(size)["blend"]
    e1, c1, p1 = full.paint(q.region, blend, return_previous=True)
    n2 = int(crops["footprint", "all"][1]["numSamples"])
    colors = np.random.RandomState(PAINT_SEED).randint(0, 1 << 32, n2, dtype=np.uint64).astype(np.uint32)
    e2, c2, p2 = e1.paint(Region(), Paint.array(), footprint=q.footprint, colors=colors, return_previous=True)
    for kind, c, prev in (("region", c1, p1), ("footprint", c2, p2)):
        assert c.tobytes() == crops[kind, "all"][1].tobytes() and len(prev) == int(c["numSamples"]) > 0, f"{what} paint {kind}: not the crop's counts"
    assert (e1.samples["color"] != full.samples["color"]).any() and (e2.samples["color"] != e1.samples["color"]).any(), f"{what} paint: a call changes nothing"
    back = e2.paint(Region(), Paint.array(), footprint=q.footprint, colors=p2)[0].paint(q.region, Paint.array(), colors=p1)[0]
    assert back.samples.tobytes() == full.samples.tobytes() and back.nodes.tobytes() == full.nodes.tobytes(), f"{what} paint: the undo is not the octree before"
    return [PaintCall(q.region, None, blend, None, e1, c1, p1), PaintCall(Region(), q.footprint, Paint.array(), colors, e2, c2, p2)]


def pack_mirror(full, what):
    """OctreeExport.pack of the full export and its unpack -> (PackedExport, pack counts, unpacked export, unpack counts): every voxel is a cell
    centre and no colour has alpha bits (rule K3), voxels come back bit for bit, leaf points within rule K8's bound."""
    px, pc = full.pack(return_counts=True)
    back, uc = px.unpack(return_counts=True)
    t, before, after = full.nodes, full.samples, back.samples
    assert int(pc["error"]) == 0 and int(pc["numInexact"]) == 0 and int(pc["numAlpha"]) == 0 and int(pc["numSamples"]) == len(before) > 0, f"{what} pack: {pc}"
    kr.assert_points_within_bound(t, before, after, full.box_min, full.box_max, what=f"{what} pack")
    vox = kr.voxel_mask(t, len(before))
    assert after[vox].tobytes() == before[vox].tobytes(), f"{what} pack: a voxel moved"
    assert (after["color"] == before["color"]).all(), f"{what} pack: a colour changed"
    return px, pc, back, uc


def assert_hits_are_brute(hits, rays, pts, what):
    """rays_ref.assert_hits_are_brute with one pass over the points per ray: hit / miss, t bit-equal to the brute-force minimum of rule 2 over
    `pts`, and the sample one of the input points that attain it."""
    rec = rays.record()
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    keys = pts.view(np.uint64).reshape(-1, 2)
    for i in range(len(rec)):
        t, ok = yr.sample_test(rec, i, x, y, z)
        if not ok.any():
            assert hits["node"][i] == abi.EXPORT_NONE and np.isposinf(hits["t"][i]), f"{what}: ray {i} hits, the brute force misses"
            continue
        tmin = t[ok].min()
        assert hits["node"][i] != abi.EXPORT_NONE and hits["t"][i:i + 1].view(np.uint64)[0] == np.float64(tmin).view(np.uint64), f"{what}: ray {i}: t {hits['t'][i]} against {tmin}"
        best = np.nonzero(ok & (t == tmin))[0]
        smp = np.ascontiguousarray(hits["sample"][i:i + 1]).view(np.uint64).reshape(2)
        assert ((keys[best, 0] == smp[0]) & (keys[best, 1] == smp[1])).any(), f"{what}: ray {i}'s sample is not an input point at the minimum"


def held_table(view, counts):
    """`view` (a cut) with the sample counts of its first len(counts) selected entries lowered to `counts`: what a receiver holds that saw
    those nodes when they were shorter -> (OctreeExport, the entries' indices)"""
    import delta_ref
    return delta_ref.lowered(view, counts=tuple(counts), floor=max(counts))


# ---- the states' shapes, and their oracle twins ----------------------------------------------------------------------------------------------------
# (what the GPU tier passes to the battery; tests/test_builder_states_io.py holds every one of them against the oracle's octree of the same input)
# (the inverse's facts: a half-space through the middle and a star around a quarter leave a node outside only where the octree is deep enough —
# the star from four terrain batches on; seen from inside, or from `closer` on 17 nodes, no node lies in the lasso whole)
_NO_CULL = dict(region_culls=False, footprint_culls=False)
SHAPES = {"A": NINE_NODES, "B": NINE_NODES, "C": Shape(), "D hotspot_150k": Shape(region_copies=False, lasso_culls=False, **_NO_CULL), "D dense_cube": Shape(), "E": Shape(),
          "E1": Shape(delta_adds=False, profile_copies=False, lasso_copies=False, **_NO_CULL), "E2": Shape(footprint_culls=False), "E3": Shape(footprint_culls=False),
          "F": Shape(), "H": Shape(), "G 600000 poisoned": Shape(), "G 600000 continued": Shape(), "G 90000 poisoned": ROOT_LEAF,
          "G 90000 continued": Shape("inside", delta_adds=False, coarser=False, profile_copies=False, lasso_copies=False, lasso_culls=False, **_NO_CULL),
          "I A": Shape("bird", footprint_culls=False), "I B": Shape("inside", delta_adds=False, lasso_copies=False, **_NO_CULL)}
G_CASES = [(600_000, 300_000, 100_000), (90_000, 30_000, 15_000)]


def d_input(name):
    """State D's inputs -> (points, box, batches, how many of them are built before the resume's export).  The hotspot in batches of 100 000
    and 50 000: its root splits in the first batch whatever the granularity (a root that ends a batch as a leaf samples itself, and what its
    voxel list keeps of that depends on where the batches end)."""
    if name == "hotspot_150k":
        pts, box, _, _ = cases.case(name)
        return pts, box, [pts[:100_000], pts[100_000:]], 1
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    return pts, box, [pts[i:i + 200_000] for i in range(0, len(pts), 200_000)], 2


def g_input(total, first, batch):
    pts, box = synthetic.terrain(total, seed=7)
    return pts, box, [pts[i:i + batch] for i in range(0, total, batch)], first // batch


def twin(name, partition=None):
    """The oracle's octree of a state's input -> (full export, the points it holds, box, the Shape the GPU tier uses, the HostOctree)"""
    key = name
    if name == "A":
        pts, box, batches = a_input()
    elif name.startswith("E"):
        pts, box, batches = e_input()
        batches, key = batches[: int(name[1:])], name if name in SHAPES else "E"
    elif name == "F":
        pts, box, batches = f_input()
        ho, u, _ = oracle_build(box, batches, capacity=f_capacity(box, batches)[0])
        taken = int(ho.stats["batchletIndex"][0])
        return export_of(ho, u), np.concatenate(batches[:taken]), box, SHAPES[key], ho
    elif name == "H":
        allpts, box, mask, mine, batches = h_input(partition)
        ho, u, _ = oracle_build(box, batches, mask=mask)
        return export_of(ho, u), mine, box, SHAPES[key], ho
    elif name.startswith("D "):
        pts, box, batches, _ = d_input(name[2:])
    elif name.startswith("G "):
        total, when = name.split()[1:]
        pts, box, batches, cut = g_input(*[c for c in G_CASES if c[0] == int(total)][0])
        batches = batches[:cut] if when == "poisoned" else batches
    elif name.startswith("I "):
        case = "terrain_4x100k" if name == "I A" else "uniform_3x40k"
        pts, box, batch, _ = cases.case(case)
        batches = cases.batches_of(case, pts, batch)
    else:
        raise KeyError(name)
    ho, u, _ = oracle_build(box, batches)
    ex = export_of(ho, u)
    return (collapse(ex) if name == "A" else ex), np.concatenate(batches), box, SHAPES[key], ho
