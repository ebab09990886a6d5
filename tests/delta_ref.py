"""Shared by the view-delta tests (tests/test_view_delta_io.py, test_gpu_view_delta.py): the camera pairs on the 3 M terrain, the uniform cube that
grows between two cuts, and the guards that keep a comparison from passing on nothing."""
import numpy as np

import cases
import oracle
import view_ref as vr
from export_ref import export_host
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import OctreeExport

# (what, the held cut's camera and view arguments, the new cut's): the first three have kept, added and dropped entries, `away` selects nothing
PAIRS = [("bird -> closer", ("bird", {}), ("closer", {})),
         ("inside -> grazing", ("inside", {}), ("grazing", {})),
         ("closer bias 0 -> 1", ("closer", {}), ("closer", {"bias": 1})),
         ("closer -> away", ("closer", {}), ("away", {}))]
MIXED = [p[0] for p in PAIRS[:3]]
CUBE_POINTS, CUBE_BATCH, CUBE_HELD_AFTER, CUBE_BIAS = 800_000, 100_000, 4, 2
_BUILT = {}


def cube_batches():
    """synthetic.uniform_cube(800 000, seed 1) in eight batches of 100 000 -> (batches, box)"""
    pts, box = synthetic.uniform_cube(CUBE_POINTS, seed=1)
    return [pts[i:i + CUBE_BATCH] for i in range(0, len(pts), CUBE_BATCH)], box


def grown_cube():
    """-> (full export after four batches, full export after all eight, box) of the oracle-built uniform cube, once per session."""
    if "cube" not in _BUILT:
        batches, box = cube_batches()
        u = cases.uniforms_for(box, np.eye(4, dtype=np.float32))
        ho = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
        ho.reset(u)
        fulls = []
        for i, b in enumerate(batches):
            ho.add_points(u, b, len(b))
            if i + 1 in (CUBE_HELD_AFTER, len(batches)):
                t, s = export_host(ho.nodes, int(ho.stats["numNodes"][0]))
                fulls.append(OctreeExport(t, s, u["boxMin"], u["boxMax"]))
        assert int(ho.stats["dbg"][0]) == 0
        _BUILT["cube"] = (fulls[0], fulls[1], box)
    return _BUILT["cube"]


def states(delta):
    """(kept, grown, added, dropped) of a ViewDelta, counted from its records."""
    s = delta.entries["state"]
    return tuple(int((s == k).sum()) for k in (abi.DELTA_KEPT, abi.DELTA_GROWN, abi.DELTA_ADDED)) + (len(delta.dropped),)


def kind_changed(delta, held):
    """The table entries whose held entry is selected with samples and of the other kind (a leaf that became an inner node, or back)."""
    e, tb, ht = delta.entries, delta.nodes, held.nodes
    found = e["held"] != abi.EXPORT_NONE
    hf = ht["flags"][np.where(found, e["held"], 0)]
    return np.nonzero(found & ((tb["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & ((hf & abi.EXPORT_FLAG_SELECTED) != 0) &
                      (((tb["flags"] ^ hf) & abi.EXPORT_FLAG_LEAF) != 0))[0]


def assert_delta_consistent(delta, held, new):
    """What every delta promises, whatever produced it: the table is the new cut's, the records obey D3-D6 among themselves, and the merge
    (rule D9, in numpy) gives the new cut back byte for byte."""
    e, tb = delta.entries, delta.nodes
    assert tb.tobytes() == new.nodes.tobytes(), "the table is not the view's"
    sel = (tb["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
    assert ((e["state"] == abi.DELTA_NONE) == ~sel).all()
    assert np.array_equal(e["numKept"].astype(np.int64) + e["numDelta"], tb["numSamples"].astype(np.int64))
    assert np.array_equal(e["firstDelta"], np.concatenate([[0], np.cumsum(e["numDelta"].astype(np.int64))[:-1]]).astype(np.uint64))
    assert int(e["numDelta"].astype(np.int64).sum()) == delta.num_samples
    c = delta.counts
    assert (int(c["numKept"]), int(c["numGrown"]), int(c["numAdded"]), int(c["numDropped"])) == states(delta)
    assert int(c["numDeltaSamples"]) == delta.num_samples and int(c["numKeptSamples"]) == int(e["numKept"].astype(np.int64).sum())
    assert int(c["numDeltaSamples"]) + int(c["numKeptSamples"]) == new.num_samples
    d = delta.dropped.astype(np.int64)
    assert (np.diff(d) > 0).all()
    merged = delta.apply(held)
    assert merged.nodes.tobytes() == new.nodes.tobytes() and merged.samples.tobytes() == new.samples.tobytes(), "the merge is not the fresh view"
    merged.validate()


def lowered(held, counts=(1, 999, 1000, 1001, -1), floor=2000):
    """`held` with numSamples lowered on the first len(counts) selected entries of more than `floor` samples (a count of -1: n - 1), firstSample
    rescanned and the sample array cut to match: what a receiver holds that got only the head of those nodes -> (OctreeExport, the entries' indices)."""
    t = held.nodes.copy()
    idx = np.nonzero(((t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (t["numSamples"] > floor))[0][: len(counts)]
    assert len(idx) == len(counts), f"only {len(idx)} selected entries above {floor} samples"
    old_first, old_n = t["firstSample"].astype(np.int64), t["numSamples"].astype(np.int64)
    for i, k in zip(idx, counts):
        t["numSamples"][i] = old_n[i] - 1 if k < 0 else k
    n = t["numSamples"].astype(np.int64)
    t["firstSample"] = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.uint64)
    keep = np.concatenate([np.arange(a, a + k) for a, k in zip(old_first, n)])
    return OctreeExport(t, held.samples[keep], held.box_min, held.box_max, held.max_level, held.select), idx
