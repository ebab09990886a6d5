"""Comparison helpers shared by the parity tests (H6-aware: see SURVEY.md §2.5)."""
import numpy as np

import cases
import oracle
from simlod_amd import abi

# fields of oracle.dump_dtype that every correct implementation must reproduce exactly
EXACT_FIELDS = ["key", "level", "X", "Y", "Z", "isLeaf", "childMask", "counter", "numPoints", "numVoxels", "numVoxelsStored",
                "countIteration", "hasGrid", "gridPopcount", "gridHash", "pointsSum", "pointsXor", "voxelPosSum", "voxelPosXor",
                "pointChunks", "voxelChunks", "name"]

# Stats fields that are deterministic for a fixed batch sequence (allocatedBytes_momentary is implementation defined)
STATS_BUILD_FIELDS = ["numNodes", "numInner", "numLeaves", "numNonemptyLeaves", "numPoints", "numVoxels", "allocatedBytes_persistent",
                      "numChunksPoints", "numChunksVoxels", "batchletIndex", "numPointsProcessed", "numAllocatedChunks", "chunkPoolSize",
                      "memCapacityReached"]
STATS_RENDER_FIELDS = ["numVisibleNodes", "numVisibleInner", "numVisibleLeaves", "numVisiblePoints", "numVisibleVoxels"]


def assert_dumps_equal(a, b, what=""):
    assert len(a) == len(b), f"{what}: node count {len(a)} != {len(b)}"
    for f in EXACT_FIELDS:
        if not np.array_equal(a[f], b[f]):
            bad = np.nonzero(np.any(np.atleast_2d((a[f] != b[f]).reshape(len(a), -1)), axis=1))[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: field {f} differs at {len(bad)} nodes; first: level={a['level'][i]} "
                                 f"XYZ=({a['X'][i]},{a['Y'][i]},{a['Z'][i]}) {a[f][i]} != {b[f][i]}")


def assert_stats_equal(a, b, fields, what=""):
    for f in fields:
        assert int(a[f]) == int(b[f]), f"{what}: Stats.{f} {int(a[f])} != {int(b[f])}"


def host_image_of(dev):
    """Download a DeviceOctree's image and rebase its pointers to the host copies."""
    nodes, pers, n, nodes_base, pers_base = dev.download_image()
    oracle.rebase_image(nodes, n, pers, nodes_base, pers_base)
    return nodes, pers, n


def voxel_colors_are_member(nodes, n, points, box_size, max_level=20):
    """Every voxel's colour must be the colour of SOME input point that falls into the voxel's cell (first-writer-wins is
    scheduling dependent).  Returns the number of voxels checked.  Nodes deeper than `max_level` are skipped:
    their cells are smaller than an fp32 position can resolve, so the cell cannot be recovered from the stored voxel position."""
    size = np.float32(max(box_size))
    X = (np.float32(2 ** 20) * points["x"] / size).astype(np.uint32)
    Y = (np.float32(2 ** 20) * points["y"] / size).astype(np.uint32)
    Z = (np.float32(2 ** 20) * points["z"] / size).astype(np.uint32)
    pX = (np.float32(2 ** 28) * points["x"] / size).astype(np.uint32)
    pY = (np.float32(2 ** 28) * points["y"] / size).astype(np.uint32)
    pZ = (np.float32(2 ** 28) * points["z"] / size).astype(np.uint32)
    checked = 0
    for i in range(n):
        nd = nodes[i]
        nv = int(nd["numVoxelsStored"])
        if nv == 0:
            continue
        lvl = int(nd["level"])
        if lvl > max_level:
            continue
        vox = oracle.gather_samples(int(nd["voxelChunks"]), nv)
        sel = ((X >> (20 - lvl)) == nd["X"]) & ((Y >> (20 - lvl)) == nd["Y"]) & ((Z >> (20 - lvl)) == nd["Z"]) if lvl > 0 else np.ones(len(points), bool)
        sh = 21 - lvl
        cell = ((pX[sel] >> sh) & 127).astype(np.uint64) | (((pY[sel] >> sh) & 127).astype(np.uint64) << 7) | (((pZ[sel] >> sh) & 127).astype(np.uint64) << 14)
        have = np.unique((cell << np.uint64(32)) | points["color"][sel].astype(np.uint64))
        node_size = size / np.float32(2.0 ** lvl)
        mn = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=np.float32) * node_size
        vc = [np.floor((vox[a] - mn[k]) / node_size * np.float32(128.0)).astype(np.int64).clip(0, 127).astype(np.uint64) for k, a in enumerate("xyz")]
        vkey = ((vc[0] | (vc[1] << np.uint64(7)) | (vc[2] << np.uint64(14))) << np.uint64(32)) | vox["color"].astype(np.uint64)
        pos = np.searchsorted(have, vkey)
        ok = (pos < len(have)) & (have[np.minimum(pos, len(have) - 1)] == vkey)
        assert ok.all(), f"node level={lvl} XYZ=({nd['X']},{nd['Y']},{nd['Z']}): {int((~ok).sum())} voxels carry a colour no point of their cell has"
        checked += nv
    return checked


# ---- which batch coloured a voxel (a voxel's colour is the colour of a point of the FIRST batch that hit its cell) ----------------
# A tagged input names its points by their colours; construction never reads a colour, so a tagged run builds the same octree (only the
# pointsSum / pointsXor hashes follow the colours), and every voxel's colour names the one input point that won its cell.

# (node = level + key X << 40 | Y << 20 | Z; cell = pX + 128 pY + 128^2 pZ of the node's grid; x, y, z = the voxel position's fp32 bits)
voxel_row_dtype = np.dtype([("level", "<u4"), ("key", "<u8"), ("cell", "<u4"), ("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("batch", "<u4")])
_ROW_ORDER = ["level", "key", "cell", "x", "y", "z", "batch"]


def tag_colors(points):
    """A copy of `points` whose colour is the global point index: each colour names exactly one input point."""
    t = np.array(points, dtype=abi.point_dtype, copy=True)
    t["color"] = np.arange(len(t), dtype=np.uint32)
    return t


def batch_of_points(batches):
    """Global point index -> index of the batch it came in (empty batches count)."""
    return np.repeat(np.arange(len(batches), dtype=np.uint32), [len(b) for b in batches])


def _voxel_rows(uniforms, nodes, n, tagged):
    """One row per stored voxel of a HOST-addressed image: (node key, cell of the winner point in the node's grid, voxel position bits,
    winner point index in `batch`).  Raises AssertionError where a winner does not lie in its voxel's node or cell."""
    out = []
    for i in np.nonzero(nodes["numVoxelsStored"][:n])[0]:
        nd = nodes[i]
        nv, lvl, X, Y, Z = int(nd["numVoxelsStored"]), int(nd["level"]), int(nd["X"]), int(nd["Y"]), int(nd["Z"])
        where = f"node level={lvl} XYZ=({X},{Y},{Z})"
        vox = oracle.gather_samples(int(nd["voxelChunks"]), nv)
        assert len(vox) == nv, f"{where}: voxel list holds {len(vox)} of its {nv} voxels"
        win = vox["color"].astype(np.int64)
        if (win >= len(tagged)).any():
            raise AssertionError(f"{where}: {int((win >= len(tagged)).sum())} voxel colours name no input point")
        cells, centres = oracle.voxel_cells(uniforms, tagged[win], lvl, X, Y, Z)
        outside = cells == 0xFFFFFFFF
        if outside.any():
            k = int(np.argmax(outside))
            raise AssertionError(f"{where}: {int(outside.sum())} voxels won by a point outside the voxel's node (first: voxel {k}, point {int(win[k])})")
        pos = np.stack([vox["x"], vox["y"], vox["z"]], axis=1)
        off = (pos.view(np.uint32) != centres.view(np.uint32)).any(axis=1)
        if off.any():
            k = int(np.argmax(off))
            raise AssertionError(f"{where}: {int(off.sum())} voxels won by a point outside the voxel's cell (first: voxel {k} at {tuple(pos[k])}, "
                                 f"point {int(win[k])} makes {tuple(centres[k])})")
        r = np.zeros(nv, dtype=voxel_row_dtype)
        r["level"] = lvl
        r["key"] = (X << 40) | (Y << 20) | Z
        r["cell"] = cells
        r["x"], r["y"], r["z"] = pos.view(np.uint32).T
        r["batch"] = win                   # (the winner, for now)
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, dtype=voxel_row_dtype)


def _sorted_rows(rows):
    return rows[np.lexsort([rows[f] for f in reversed(_ROW_ORDER)])]


def replay_first_hits(uniforms, batches, persistent_bytes=None):
    """Run `batches` (tagged) through the port oracle ONE at a time.  The oracle appends a node's voxels in batch order
    (simlod_oracle.c insertVoxels: slot = numVoxelsStored++), so slot i of a node was made by the first batch after which its numVoxelsStored
    exceeds i.  Returns (the HostOctree as the last batch it took left it, the first-hit table: voxel_row_dtype rows sorted by
    (node, cell, position bits, batch) — every (node, position) group's `batch` column is the sorted list of its first-hit batches b*).
    A cell can hold several voxels: the root's grid is cleared when the root splits.  A batch the memory guard refuses ends the replay."""
    u = np.ascontiguousarray(uniforms).reshape(1)
    tagged = np.concatenate(batches) if len(batches) else np.zeros(0, dtype=abi.point_dtype)
    assert np.array_equal(tagged["color"], np.arange(len(tagged), dtype=np.uint32)), "replay_first_hits wants tag_colors() points"
    cap = int(u["persistentBufferCapacity"][0])
    ref = oracle.HostOctree("port", persistent_bytes=persistent_bytes or min(cap, 4 << 30), ring_slots=abi.BATCH_STREAM_SIZE)
    ref.reset(u)
    prev = np.zeros(0, dtype=np.int64)
    ev_node, ev_old, ev_new, ev_batch = [], [], [], []
    for b, pts in enumerate(batches):
        ref.upload(pts)
        ref.construct(u)                   # (nothing else is pending: the launch takes this batch, or the memory guard refuses it)
        assert ref.last_error() == 0, f"oracle error {ref.last_error()} in batch {b}"
        if int(ref.stats["batchletIndex"][0]) != b + 1:
            break
        cur = ref.nodes["numVoxelsStored"][: int(ref.stats["numNodes"][0])].astype(np.int64)
        old = np.zeros_like(cur)
        old[: len(prev)] = prev
        ch = np.nonzero(cur != old)[0]
        ev_node.append(ch); ev_old.append(old[ch]); ev_new.append(cur[ch]); ev_batch.append(np.full(len(ch), b))
        prev = cur
    nn = int(ref.stats["numNodes"][0])
    rows = _voxel_rows(u, ref.nodes, nn, tagged)
    if len(rows):
        node, old, new, bat = (np.concatenate(v) for v in (ev_node, ev_old, ev_new, ev_batch))
        cnt = new - old
        assert (cnt > 0).all(), "numVoxelsStored shrank"
        # b* per (node, slot), in the order _voxel_rows lists the voxels: nodes by index, slots ascending (a node's events come in batch order)
        order = np.argsort(node, kind="stable")
        bstar = np.repeat(bat[order], cnt[order])
        assert len(bstar) == len(rows)
        rows["batch"] = bstar
    return ref, _sorted_rows(rows)


def first_hit_batches(uniforms, batches):
    """The first-hit table of replay_first_hits (see there)."""
    return replay_first_hits(uniforms, batches)[1]


def assert_voxel_winners(nodes, n, tagged, batch_of_point, first_hit, bound, uniforms):
    """Batch-aware colour check of a HOST-addressed image built from `tagged` points (tag_colors).  Every voxel's winner must lie in the
    voxel's node and cell (oracle_voxel_cells: the oracle's own quantization, every level); grouped by (node, cell, position) and sorted on
    both sides, the voxels must pair up one to one with the first-hit table's, and the batch of each winner must be <= bound(b*) of its
    partner (bound: numpy array of b* -> array of the latest batch allowed; `lambda b: b` is the reference's rule).  Returns the number of
    voxels checked."""
    rows = _voxel_rows(uniforms, nodes, n, tagged)
    rows["batch"] = batch_of_point[rows["batch"].astype(np.int64)]
    rows = _sorted_rows(rows)
    same = len(rows) == len(first_hit)
    if same:
        diff = np.zeros(len(rows), bool)
        for f in _ROW_ORDER[:-1]:
            diff |= rows[f] != first_hit[f]
        same = not diff.any()
    if not same:
        ca, cb = {}, {}
        for c, t in ((ca, rows), (cb, first_hit)):
            for k in t[_ROW_ORDER[:3]].tolist():
                c[k] = c.get(k, 0) + 1
        bad = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
        k = bad[0] if bad else (0, 0, 0)
        raise AssertionError(f"voxel counts per (node, cell) differ from the oracle's at {len(bad)} cells ({len(rows)} voxels, oracle {len(first_hit)}); "
                             f"first: level {k[0]} XYZ key {k[1]:#x} cell {k[2]}: {ca.get(k, 0)} != {cb.get(k, 0)}")
    allowed = np.asarray(bound(first_hit["batch"].astype(np.int64)))
    late = rows["batch"].astype(np.int64) > allowed
    if late.any():
        i = int(np.argmax(late))
        raise AssertionError(f"{int(late.sum())} of {len(rows)} voxels are coloured from a later batch than the bound allows; first: level "
                             f"{int(rows['level'][i])} XYZ key {int(rows['key'][i]):#x} cell {int(rows['cell'][i])}: batch {int(rows['batch'][i])}, first hit {int(first_hit['batch'][i])}, "
                             f"allowed <= {int(allowed[i])}")
    return len(rows)


def late_voxels(nodes, n, tagged, batch_of_point, first_hit, uniforms):
    """How many voxels are coloured from a later batch than the first that hit their cell (the pairing of assert_voxel_winners)."""
    rows = _voxel_rows(uniforms, nodes, n, tagged)
    rows["batch"] = batch_of_point[rows["batch"].astype(np.int64)]
    rows = _sorted_rows(rows)
    assert len(rows) == len(first_hit)
    return int((rows["batch"] > first_hit["batch"]).sum()), len(rows)


def points_multiset_hash(pts):
    """(sum, xor) order-independent hash of a set of 16-byte points — the same mixer as oracle_dump's pointsSum / pointsXor."""
    w = pts.view(np.uint32).reshape(-1, 4).astype(np.uint64)

    def mix(x):
        x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xbf58476d1ce4e5b9); x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))
    with np.errstate(over="ignore"):
        a = (w[:, 0] << np.uint64(32)) | w[:, 1]
        b = (w[:, 2] << np.uint64(32)) | w[:, 3]
        h = mix(a ^ mix(b + np.uint64(0x9e3779b97f4a7c15)))
        return np.uint64(h.sum()), np.bitwise_xor.reduce(mix(h + np.uint64(1)))


def oracle_frame(nodes, nn, u):
    """The oracle's rasteriser on a HOST-addressed image -> (pre-EDL framebuffer uint64[H*W], EDL'd RGBA8 uint32[H*W], Stats record, visible-node records)."""
    import ctypes
    Wd, Hd = int(u["width"]), int(u["height"])
    fb = np.zeros(Wd * Hd, dtype=np.uint64)
    col = np.zeros(Wd * Hd, dtype=np.uint32)
    vis = np.zeros(abi.MAX_VISIBLE_NODES, dtype=abi.node_dtype)
    stats = np.zeros(1, dtype=abi.stats_dtype)
    stats["numNodes"] = nn
    uu = np.ascontiguousarray(u).reshape(1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    oracle.port_lib().oracle_render(None, p(uu), p(nodes), p(stats), p(fb), p(col), p(vis), 1)
    return fb, col, stats[0], vis[: int(stats["numVisibleNodes"][0])].copy()


def node_keys(rec):
    """level << 60 | X << 40 | Y << 20 | Z of Node (or export table) records."""
    return ((rec["level"].astype(np.uint64) << np.uint64(60)) | (rec["X"].astype(np.uint64) << np.uint64(40)) | (rec["Y"].astype(np.uint64) << np.uint64(20)) |
            rec["Z"].astype(np.uint64))


def assert_frame_equals_oracle(dev, nodes, nn, u, what, floor):
    """The frame the device just drew from `u` against the oracle's on the same image: render Stats equal, pre-EDL framebuffer bit-identical,
    more than `floor` pixels drawn, RGBA8 within 1 per channel (log2 / exp from different libms).  -> (device fb, colour, oracle Stats, visible records)."""
    Wd, Hd = int(u["width"]), int(u["height"])
    fb_dev, col_dev, ds = dev.framebuffer(Wd, Hd), dev.color(Wd, Hd), dev.read_stats()
    assert int(ds["dbg"]) == 0, f"{what}: device error bits {int(ds['dbg']):#x}"
    fb, col, st, vis = oracle_frame(nodes, nn, u)
    assert_stats_equal(ds, st, STATS_RENDER_FIELDS, what)
    diff = np.nonzero(fb_dev != fb)[0]
    assert len(diff) == 0, f"{what}: {len(diff)} pixels differ, first {diff[:5]}: dev {fb_dev[diff[:5]]} oracle {fb[diff[:5]]}"
    if floor is not None:
        assert int((fb != abi.CLEAR_PIXEL).sum()) > floor, f"{what}: the case must draw something"
    assert int(np.abs(col_dev.view(np.uint8).astype(np.int16) - col.view(np.uint8).astype(np.int16)).max()) <= 1, f"{what}: RGBA8 differs by more than 1"
    return fb_dev, col_dev, st, vis


# -- what the GPU query tests (region, rays, neighbours) build their octrees with ------------------------------------------------------
def _device(**kw):
    from simlod_amd.runtime import DeviceOctree
    kw.setdefault("persistent_bytes", 2 << 30)
    kw.setdefault("max_pixels", 1920 * 1080)
    dev = DeviceOctree("cuda:0", **kw)
    # nothing may trust bytes it did not write (tests/test_gpu_parity.py _device)
    dev.momentary.fill_(0xA5); dev.render_buffer.fill_(0xA5); dev.persistent.fill_(0xA5)
    return dev


def _ingest(dev, u, batches):
    for b in batches:
        if dev.uploaded_host - dev.processed() >= dev.ring_slots:
            dev.drain(u)
        dev.upload(b)
    dev.drain(u)
    assert int(dev.read_stats()["dbg"]) == 0


def _build(name, offset=None):
    dev = _device()
    if offset is None:
        pts, box, batch, T = cases.case(name)
        u = dev.uniforms(cases.W, cases.H, T, box)
    else:
        pts, box_min, box, batch = cases.shifted(name, offset)
        u = dev.uniforms(cases.W, cases.H, cases.shifted_cam(box, offset), box, box_min=box_min)
    dev.reset(u)
    _ingest(dev, u, cases.batches_of(name, pts, batch))
    return dev, u, pts, box


def _chunks(export):
    """The chunk items of an export's table: ceil(numSamples / 1000) per node."""
    ns = export.nodes["numSamples"].astype(np.int64)
    return int(((ns + abi.POINTS_PER_CHUNK - 1) // abi.POINTS_PER_CHUNK).sum())
