"""Shared by the region-query tests: the regions they use, the brute-force filter of an input array (which never went through an octree),
exact multiset comparison of 16-byte samples, and octrees built on the host by the oracle."""
import numpy as np

import cases
import oracle
from export_ref import export_host
from simlod_amd import abi
from simlod_amd.octree_io import OctreeExport, Region

NORMAL = (0.6, 0.8, 0.1)
REGION_NAMES = ["oblique", "slab", "box", "none", "miss"]


def region(kind, box, box_min=(0, 0, 0)):
    """The test regions, placed relative to the box [box_min, box_min + box]: an oblique half-space through the centre, a slab around it,
    an x/y box of 30-70 % x 20-90 % of the extents, no plane at all, a half-space that misses the box."""
    box = np.asarray(box, dtype=np.float64)
    mn = np.asarray(box_min, dtype=np.float64)
    n = np.asarray(NORMAL)
    c = float(n @ (mn + box / 2))
    if kind == "oblique":
        return Region.from_planes([[*n, -c]])
    if kind == "slab":
        h = 0.2 * float(box.max())
        return Region.from_planes([[*n, -c + h], [*(-n), c + h]])
    if kind == "box":
        return Region.from_box((mn[0] + 0.3 * box[0], mn[1] + 0.2 * box[1], mn[2] - 1.0), (mn[0] + 0.7 * box[0], mn[1] + 0.9 * box[1], mn[2] + box[2] + 1.0))
    if kind == "none":
        return Region()
    if kind == "miss":
        return Region.from_planes([[1.0, 0.0, 0.0, -(float(mn[0]) + 3.0 * float(box.max()))]])
    raise KeyError(kind)


def brute_mask(region_, pts):
    """Rule 3 on raw points: ((nx*x + ny*y) + nz*z) + d >= 0 for every plane, in float64."""
    x, y, z = (pts[a].astype(np.float64) for a in ("x", "y", "z"))
    ok = np.ones(len(pts), bool)
    for nx, ny, nz, d in region_.planes.astype(np.float64):
        ok &= ((nx * x + ny * y) + nz * z) + d >= 0
    return ok


def sorted_samples(pts):
    """The samples as (n, 2) uint64 rows in sorted order: equal arrays <=> equal multisets."""
    w = np.ascontiguousarray(pts).view(np.uint64).reshape(-1, 2)
    return w[np.lexsort((w[:, 1], w[:, 0]))]


def assert_same_multiset(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} samples, expected {len(want)}"
    assert np.array_equal(sorted_samples(got), sorted_samples(want)), f"{what}: the samples differ as multisets"


def host_octree(name=None, pts=None, box=None, batch=None, box_min=(0, 0, 0), batches=None, export=True):
    """An octree built by the oracle's port from a case of tests/cases.py (or from `pts`, or from `batches` of unequal sizes)
    -> (full export as OctreeExport, points, box, HostOctree).
    With `box_min` the case's points are moved by it (cases.shifted) and the box starts there.  export=False: no export (None in its place),
    for an image export_host cannot walk as it stands."""
    if name is not None:
        pts, box, batch, T = cases.case(name)
        if tuple(box_min) != (0, 0, 0):
            pts, box_min, box, batch = cases.shifted(name, box_min)
        batches = cases.batches_of(name, pts, batch)
    elif batches is not None:
        pts = np.concatenate(batches)
    else:
        batches = [pts[i:i + batch] for i in range(0, len(pts), batch)]
    u = cases.uniforms_for(box, np.eye(4, dtype=np.float32), box_min=box_min)
    ho = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ho.reset(u)
    for b in batches:
        if len(b):
            ho.add_points(u, b, len(b))
    assert int(ho.stats["dbg"][0]) == 0
    if not export:
        return None, pts, box, ho
    t, s = export_host(ho.nodes, int(ho.stats["numNodes"][0]))
    return OctreeExport(t, s, u["boxMin"], u["boxMax"]), pts, box, ho
