"""CPU tier: the export table's layout, the file format of simlod_amd/octree_io.py and its validation, and the host restatement of the export
(tests/export_ref.py) on an octree built by the oracle."""
import os
import re

import numpy as np
import pytest

import cases
import oracle
from export_ref import export_host
from simlod_amd import abi
from simlod_amd.octree_io import OctreeExport, validate_table
from util import points_multiset_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (10.0, 20.0, 30.0)


def test_export_node_dtype_matches_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    offs = dict(re.findall(r"offsetof\(SimlodExportNode, (\w+)\) == (\d+)", src))
    assert len(offs) >= 7
    for f, o in offs.items():
        assert abi.export_node_dtype.fields[f][1] == int(o), f
    assert int(re.search(r"sizeof\(SimlodExportNode\) == (\d+)", src).group(1)) == abi.export_node_dtype.itemsize
    assert int(re.search(r"sizeof\(SimlodExportCounts\) == (\d+)", src).group(1)) == abi.export_counts_dtype.itemsize
    assert int(re.search(r"offsetof\(SimlodExportCounts, numSamples\) == (\d+)", src).group(1)) == abi.export_counts_dtype.fields["numSamples"][1]
    assert int(re.search(r"#define SIMLOD_ERR_IMPORT (0x[0-9a-f]+)u", src).group(1), 16) == abi.SIMLOD_ERR_IMPORT


def test_export_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_export_buffer_min_bytes", "simlod_export_octree", "simlod_import_octree"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    # the scratch bound grows with both capacities (one 32-byte copy item per chunk)
    a = L.simlod_export_buffer_min_bytes(100, 0)
    assert L.simlod_export_buffer_min_bytes(100, 1_000_000) >= a + 1000 * 32 and L.simlod_export_buffer_min_bytes(200, 0) > a


def test_scratch_bounds_are_exactly_the_layouts(built_libs):
    """The three scratch bounds are a contract with callers: each is pinned to the layout it states, region by region (csrc/export_common.inc
    Layout, export_region.inc QueryLayout, export_pairs.inc PairLayout): a 256-byte header (two for the pair queries), every array rounded
    up to 256 bytes, then 32 bytes per chunk item, per pair, and 16 per further thousand candidates."""
    from simlod_amd import runtime
    L = runtime.lib()

    def a(v):
        return (v + 255) & ~255

    def items(cap, bound):
        return (bound // 1000 + cap + 1) * 32

    for cap in (0, 1, 64, 100, 4425):
        q, f = a(4 * cap), a(4 * cap + 4)
        for bound in (0, 999, 1000, 36_000_000):
            assert L.simlod_export_buffer_min_bytes(cap, bound) == 256 + 2 * q + f + items(cap, bound), (cap, bound)
            assert L.simlod_query_buffer_min_bytes(cap, bound) == 256 + 3 * q + f + items(cap, bound), (cap, bound)
            for rays in (1, 64, 4096):
                for pairs, cand in ((0, 0), (3, 68_019)):
                    want = (512 + 5 * q + f + a(40 * cap) + a(8 * cap + 8) + a(4 * rays) + a(8 * rays + 8) + items(cap, bound)
                            + 32 * pairs + 16 * (cand // 1000))
                    assert L.simlod_rays_buffer_min_bytes(cap, bound, rays, pairs, cand) == want, (cap, bound, rays, pairs, cand)


def _table(spec):
    """A breadth-first table from {octant: subtree} dicts (the root is `spec`); every node gets (level + 1) * 3 samples."""
    rows, queue = [], [(spec, abi.EXPORT_NONE, 0, 0, 0, 0)]
    while queue:
        nxt = []
        for sub, parent, lvl, x, y, z in queue:
            t = len(rows)
            mask = sum(1 << k for k in sub)
            rows.append([lvl, x, y, z, parent, abi.EXPORT_NONE, mask, 0 if mask else abi.EXPORT_FLAG_LEAF | abi.EXPORT_FLAG_SELECTED, (lvl + 1) * 3])
            for k in sorted(sub):
                nxt.append((sub[k], t, lvl + 1, 2 * x + (k >> 2 & 1), 2 * y + (k >> 1 & 1), 2 * z + (k & 1)))
        queue = nxt
    # firstChild: children of a node follow the children of the nodes before it
    nextc = 1
    for r in rows:
        if r[6]:
            r[5] = nextc
            nextc += bin(r[6]).count("1")
    t = np.zeros(len(rows), dtype=abi.export_node_dtype)
    for i, r in enumerate(rows):
        for f, v in zip(("level", "X", "Y", "Z", "parent", "firstChild", "childMask", "flags", "numSamples"), r):
            t[i][f] = v
    t["firstSample"] = np.concatenate([[0], np.cumsum(t["numSamples"].astype(np.uint64))[:-1]])
    return t


def _export():
    t = _table({0: {}, 5: {1: {}, 7: {}}, 6: {}})
    rs = np.random.RandomState(3)
    s = np.zeros(int(t["numSamples"].sum()), dtype=abi.point_dtype)
    s["x"], s["y"], s["z"] = rs.rand(3, len(s)).astype(np.float32)
    s["color"] = rs.randint(0, 2 ** 32, len(s), dtype=np.uint64).astype(np.uint32)
    return OctreeExport(t, s, (0, 0, 0), BOX, 20, "all")


def test_save_load_roundtrip(tmp_path):
    ex = _export().validate()
    assert ex.num_nodes == 6 and ex.nodes["level"].max() == 2
    p = tmp_path / "a.simlodx"
    ex.save(p)
    ld = OctreeExport.load(p)
    assert ld.nodes.tobytes() == ex.nodes.tobytes() and ld.samples.tobytes() == ex.samples.tobytes()
    assert ld.box_max == tuple(np.float32(BOX).tolist()) and ld.max_level == 20 and ld.select == abi.EXPORT_ALL
    q = tmp_path / "b.simlodx"
    ld.save(q)
    assert p.read_bytes() == q.read_bytes()
    assert len(p.read_bytes()) == 64 + 6 * 40 + len(ex.samples) * 16


def _corrupt(tmp_path, fn, name):
    p = tmp_path / name
    _export().save(p)
    raw = bytearray(p.read_bytes())
    fn(raw)
    p.write_bytes(bytes(raw))
    return p


def _set(raw, entry, field, value):
    off = 64 + entry * 40 + abi.export_node_dtype.fields[field][1]
    dt = abi.export_node_dtype.fields[field][0]
    raw[off: off + dt.itemsize] = np.array([value], dtype=dt).tobytes()


@pytest.mark.parametrize("what,fn,msg", [
    ("magic", lambda r: r.__setitem__(slice(0, 1), b"X"), "magic"),
    ("version", lambda r: r.__setitem__(slice(8, 12), np.uint32(2).tobytes()), "version"),
    ("truncated", lambda r: r.__delitem__(slice(len(r) - 16, len(r))), "bytes"),
    ("child_range", lambda r: _set(r, 2, "firstChild", 60), "child index out of range"),
    ("scan", lambda r: _set(r, 3, "firstSample", 1), "scan"),
    ("level", lambda r: _set(r, 4, "level", 3), "level"),
    ("coordinate", lambda r: _set(r, 4, "Y", 7), "coordinate"),
])
def test_load_rejects(tmp_path, what, fn, msg):
    p = _corrupt(tmp_path, fn, what)
    with pytest.raises(ValueError, match=msg):
        OctreeExport.load(p)


def test_validate_rejects_in_memory():
    ex = _export()
    for field, entry, value in (("parent", 1, 1), ("childMask", 0, 0x21), ("reserved", 1, 1), ("numSamples", 5, 0)):
        t = ex.nodes.copy()
        t[entry][field] = value
        with pytest.raises(ValueError):
            validate_table(t, ex.num_samples)


@pytest.fixture(scope="module")
def host_octree():
    pts, box, batch, T = cases.case("terrain_4x100k")
    u = cases.uniforms_for(box, T)
    ho = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ho.reset(u)
    ho.add_points(u, pts, batch)
    return ho, pts, box


def test_host_restatement_on_oracle_octree(host_octree):
    ho, pts, box = host_octree
    n = int(ho.stats["numNodes"][0])
    t, s = export_host(ho.nodes, n)
    assert len(t) == n and len(s) == int(ho.stats["numPoints"][0]) + int(ho.stats["numVoxels"][0])
    OctreeExport(t, s, (0, 0, 0), box).validate()
    tc, sc = export_host(ho.nodes, n, 20, abi.EXPORT_CUT)
    assert tc.tobytes() != t.tobytes() and len(sc) == len(pts)
    assert points_multiset_hash(sc) == points_multiset_hash(pts)
    OctreeExport(tc, sc, (0, 0, 0), box, 20, "cut").validate()
    # a truncated table is a table too: nodes of levels 0..2, the inner nodes at level 2 carrying their voxels
    t2, s2 = export_host(ho.nodes, n, 2, abi.EXPORT_CUT)
    assert t2["level"].max() == 2 and (t2["childMask"][t2["level"] == 2] == 0).all()
    OctreeExport(t2, s2, (0, 0, 0), box, 2, "cut").validate()
