"""Test-side restatement of simlod_export_octree (include/simlod_hip.h, "octree export / import") on a HOST-addressed octree image: the
breadth-first walk over Node.children and the samples gathered along the chunk lists (oracle.gather_samples).  Device exports are compared
against it byte for byte: both read the same image's lists in list order."""
import numpy as np

import oracle
from simlod_amd import abi


def export_host(nodes, num_nodes, max_level=20, select=abi.EXPORT_ALL):
    """-> (table as abi.export_node_dtype, samples as abi.point_dtype) of the image `nodes` (pointers rebased to the host copy, as
    oracle.rebase_image leaves them, or an oracle.HostOctree's own arrays)."""
    nodes = nodes.view(abi.node_dtype)
    base = nodes.ctypes.data
    ml = min(int(max_level), abi.MAX_DEPTH)
    src = [0]                  # table index -> node index
    parent = [abi.EXPORT_NONE]
    rows = []
    t = 0
    while t < len(src):
        nd = nodes[src[t]]
        ch = [int(c) for c in nd["children"]]
        leaf = not any(ch)
        mask, first = 0, abi.EXPORT_NONE
        if nd["level"] < ml:
            for k, c in enumerate(ch):
                if c:
                    off = c - base
                    assert off % abi.node_dtype.itemsize == 0 and 0 <= off // abi.node_dtype.itemsize < num_nodes, "child outside the node array"
                    if first == abi.EXPORT_NONE:
                        first = len(src)
                    mask |= 1 << k
                    src.append(off // abi.node_dtype.itemsize)
                    parent.append(t)
        if select == abi.EXPORT_ALL:
            sel = True
        elif select == abi.EXPORT_CUT:
            sel = leaf or int(nd["level"]) == ml
        else:   # the disjunct rule of kernel_render (render.cu:905-935) over the bytes the last frame wrote
            p_large = parent[t] != abi.EXPORT_NONE and nodes[src[parent[t]]]["isLarge"] != 0
            sel = nd["visible"] != 0 and (leaf if nd["isLarge"] != 0 else p_large)
        ns = (int(nd["numPoints"]) if leaf else int(nd["numVoxels"])) if sel else 0
        rows.append((int(nd["level"]), int(nd["X"]), int(nd["Y"]), int(nd["Z"]), parent[t], first, mask,
                     (abi.EXPORT_FLAG_LEAF if leaf else 0) | (abi.EXPORT_FLAG_SELECTED if sel else 0), ns))
        t += 1
    assert ml < abi.MAX_DEPTH or len(src) == num_nodes, f"{len(src)} nodes reached from the root, the image has {num_nodes}"
    table = np.zeros(len(rows), dtype=abi.export_node_dtype)
    for i, r in enumerate(rows):
        for f, v in zip(("level", "X", "Y", "Z", "parent", "firstChild", "childMask", "flags", "numSamples"), r):
            table[i][f] = v
    table["firstSample"] = np.concatenate([[0], np.cumsum(table["numSamples"].astype(np.uint64))[:-1]]).astype(np.uint64)
    parts = []
    for i in range(len(rows)):
        ns = int(table[i]["numSamples"])
        if ns == 0:
            continue
        nd = nodes[src[i]]
        head = nd["points"] if table[i]["flags"] & abi.EXPORT_FLAG_LEAF else nd["voxelChunks"]
        got = oracle.gather_samples(int(head), ns)
        assert len(got) == ns, "a chunk list is shorter than its count"
        parts.append(got)
    samples = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)
    return table, samples


def keys_of(table):
    """(level, X, Y, Z) of each entry as one integer per entry, the key oracle.dump_image sorts by."""
    t = table.view(abi.export_node_dtype)
    return (t["level"].astype(np.uint64) << np.uint64(60)) | (t["X"].astype(np.uint64) << np.uint64(40)) | (t["Y"].astype(np.uint64) << np.uint64(20)) | t["Z"].astype(np.uint64)


def entry_index(table):
    """{(level, X, Y, Z): table index}.  (keys_of keeps four bits of the level: from level 16 on it wraps, which sorting a dump survives and a
    lookup by a Python integer does not.)"""
    t = table.view(abi.export_node_dtype)
    return {(int(l), int(x), int(y), int(z)): i for i, (l, x, y, z) in enumerate(zip(t["level"], t["X"], t["Y"], t["Z"]))}
