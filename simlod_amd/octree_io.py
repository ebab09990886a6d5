"""A built octree in a pointer-free form: the export table and sample array of simlod_export_octree (include/simlod_hip.h, "octree
export / import"), its host-side validation, and a file format for it.

File format (little-endian throughout):

    offset  bytes  field
         0      8  magic b"SIMLODX\\0"
         8      4  version (1)
        12      4  select (0 all, 1 cut, 2 visible, 3 a region query: a crop)
        16      4  max_level (20: every level)
        20      4  header bytes (64)
        24      8  numNodes
        32      8  numSamples
        40     12  box_min, 3 x float32
        52     12  box_max, 3 x float32
        64          numNodes x 40-byte SimlodExportNode (abi.export_node_dtype)
                    numSamples x 16-byte SimlodPoint (abi.point_dtype)

`load` checks the header, the file size and the table (`validate`) before anything reaches a device.

Region queries (include/simlod_hip.h, "region queries"): `Region` holds the half-spaces, and `OctreeExport.crop` is the host mirror of
simlod_query_region — every rule restated in numpy float64, which reproduces the device's fp64 arithmetic bit for bit.

Footprint queries (include/simlod_hip.h, "footprint queries"): `Footprint` holds the polygon and the affine map into its plane,
`OctreeExport.crop(region, footprint=...)` is the host mirror of simlod_query_footprint, in the same float64 operation order.

Lasso queries (include/simlod_hip.h, "lasso queries"): `Lasso` holds a polygon on the screen of a perspective camera and the three rows that
project a point onto it, `classify_lasso` is rules L2-L4, and `OctreeExport.crop / paint / summarize(lasso=...)` are the host mirrors of
simlod_query_lasso, simlod_paint_lasso and simlod_query_summary_lasso, in the same float64 operation order.

Paint regions (include/simlod_hip.h, "paint regions"): `Paint` holds the mode and its parameters, `OctreeExport.paint` is the host mirror of
simlod_paint_region — the same export with the colours of crop's samples changed, and the colours they had.

Summary queries (include/simlod_hip.h, "summary queries"): `OctreeExport.summarize` is the host mirror of simlod_query_summary — crop's samples
reduced to one record in numpy float64 and integers —, `Summary` wraps that record (extent, centroid, covariance, the range and the equalised
table of a height ramp) and `Paint.ramp_from` turns one into a RAMP paint.

Compare queries (include/simlod_hip.h, "compare queries"): `Compare` holds the radius, the thresholds, the colour table and the budget,
`compare_samples` is the host mirror of simlod_compare_samples — two sample arrays in, records, colours and the summary record out, rules
C1-C5 in numpy float64 and integers —, `OctreeExport.compare` applies it to two exports and `CompareResult` is what
DeviceOctree.compare_region returns.

Cluster queries (include/simlod_hip.h, "cluster queries"): `Cluster` holds the radius, minNeighbours, minClusterSize, the colour table and the
budget, `cluster_samples` is the host mirror of simlod_cluster_samples — rules K1-K10 on compare_samples' pairs, the components by passing the
minimum label along the core links with pointer jumping until nothing changes, numpy only —, `OctreeExport.cluster` applies it to an export
and `ClusterResult` is what DeviceOctree.cluster_region returns.

Surface queries (include/simlod_hip.h, "surface queries"): `Surface` holds the radius, the thresholds, the colour table, the light and the
orientation, `surface_samples` is the host mirror of simlod_surface_samples — rules N1-N10 on compare_samples' pairs, the sums in int64, the
rest in numpy float64 —, `OctreeExport.surface` applies it to an export and `SurfaceResult` is what DeviceOctree.surface_region returns.

Profile queries (include/simlod_hip.h, "profile queries"): `Profile` holds the polyline, the half-width and the three affine maps,
`OctreeExport.profile` is the host mirror of simlod_query_profile — samples and records — and `classify_profile` of its rule P3.

View queries (include/simlod_hip.h, "view queries"): `OctreeExport.view` (on a full export) is the host mirror of simlod_query_view and
`view_geometry` of its rules V2 and V3 — the rasteriser's visibility arithmetic in numpy float32, in the device's operation order.

View deltas (include/simlod_hip.h, "view deltas"): `OctreeExport.view_delta` is the host mirror of simlod_query_view_delta — `view` plus the
rules D2-D6 (`delta_between`) — and `ViewDelta.apply` of simlod_merge_view_delta (rule D9).

Packed samples (include/simlod_hip.h, "packed samples"): `pack_samples` / `unpack_samples` are the host mirror of simlod_pack_samples /
simlod_unpack_samples (rules K0-K8, numpy float64 / float32 in the device's operation order), `OctreeExport.pack` and `ViewDelta.pack` apply them,
and `PackedExport` has a file format of its own: magic b"SIMLODP\\0", version 1, the same 64-byte header (numSamples counts the 8-byte records)
and table, then numSamples x 8 bytes; `PackedExport.load` checks header, size and table like `OctreeExport.load`.

Ray queries (include/simlod_hip.h, "ray queries"): `Rays` holds a batch of SimlodRay records, `OctreeExport.cast` (on a full export) and
`OctreeExport.cast_selected` (on any export) are the host mirror of simlod_query_rays, in the same float64 operation order.

Neighbour queries (include/simlod_hip.h, "neighbour queries"): `Spheres` holds a batch of SimlodSphere records, `OctreeExport.neighbours` (on a
full export) and `OctreeExport.neighbours_selected` (on any export) are the host mirror of simlod_query_neighbours, built the same way.
"""
import numpy as np
import torch

from . import abi

MAGIC = b"SIMLODX\0"
VERSION = 1
HEADER_BYTES = 64
header_dtype = np.dtype({
    "names": ["magic", "version", "select", "max_level", "header_bytes", "numNodes", "numSamples", "box_min", "box_max"],
    "formats": ["S8", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", ("<f4", 3), ("<f4", 3)],
    "offsets": [0, 8, 12, 16, 20, 24, 32, 40, 52],
    "itemsize": HEADER_BYTES,
})

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def _as_bytes_tensor(a):
    if isinstance(a, torch.Tensor):
        return a.reshape(-1).view(torch.uint8)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


class OctreeExport:
    """The table (numNodes x abi.export_node_dtype) and the samples (numSamples x abi.point_dtype) as uint8 tensors on the host or on a device,
    with what is needed to render them again: the box of the uniforms they were built with, and which part of the octree they hold."""

    def __init__(self, table, samples, box_min, box_max, max_level=20, select=abi.EXPORT_ALL):
        self.table_tensor = _as_bytes_tensor(table)
        self.samples_tensor = _as_bytes_tensor(samples)
        if self.table_tensor.numel() % abi.export_node_dtype.itemsize or self.samples_tensor.numel() % abi.point_dtype.itemsize:
            raise ValueError("table / samples are not whole records")
        self.box_min = tuple(float(v) for v in np.asarray(box_min, dtype=np.float32).reshape(3))
        self.box_max = tuple(float(v) for v in np.asarray(box_max, dtype=np.float32).reshape(3))
        self.max_level = int(max_level)
        self.select = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)
        self._nodes = self._samples = None

    @property
    def num_nodes(self):
        return self.table_tensor.numel() // abi.export_node_dtype.itemsize

    @property
    def num_samples(self):
        return self.samples_tensor.numel() // abi.point_dtype.itemsize

    @property
    def device(self):
        return self.table_tensor.device

    @property
    def nodes(self):
        """The table as a numpy array of abi.export_node_dtype (copied to the host once)."""
        if self._nodes is None:
            self._nodes = self.table_tensor.cpu().numpy().view(abi.export_node_dtype)
        return self._nodes

    @property
    def samples(self):
        """The samples as a numpy array of abi.point_dtype (copied to the host once)."""
        if self._samples is None:
            self._samples = self.samples_tensor.cpu().numpy().view(abi.point_dtype)
        return self._samples

    def to(self, device):
        return OctreeExport(self.table_tensor.to(device), self.samples_tensor.to(device), self.box_min, self.box_max, self.max_level, self.select)

    def validate(self, buildable=False):
        """The host-side mirror of the checks simlod_import_octree runs on the device; raises ValueError naming the first that fails.
        buildable=True: also those of simlod_import_octree_buildable — a full export (select "all", max_level 20) of an octree the builder made
        (validate_table(buildable=True))."""
        if buildable:
            if self.select != abi.EXPORT_ALL:
                raise ValueError(f"not a full export (select {self.select}): a resumable octree needs every node's samples")
            if self.max_level < abi.MAX_DEPTH:
                raise ValueError(f"a truncated export (max_level {self.max_level}): a resumable octree needs every level")
        validate_table(self.nodes, self.num_samples, buildable)
        return self

    @property
    def is_buildable(self):
        """Whether import_octree(buildable=True) accepts this export (validate(buildable=True) passes)."""
        try:
            self.validate(buildable=True)
        except ValueError:
            return False
        return True

    def crop(self, region, max_level=None, select="all", return_counts=False, footprint=None, profile=None, test_every_sample=False, return_index=False, lasso=None,
             invert=False):
        """The host mirror of simlod_query_region: what the device returns for `region` on the octree this FULL export (select "all", max level
        20; anything else ValueError) was taken from, as an OctreeExport on the host — and, return_counts, the SimlodQueryCounts record too.
        footprint (a Footprint): the mirror of simlod_query_footprint — rules F1-F4 on top of the planes; rule F5's promise is asserted for
        every copied and every outside node.
        profile (a Profile): the samples of simlod_query_profile (OctreeExport.profile adds the records) — rules P1 and P3 on top of the planes;
        rule P4's promise is asserted likewise.  test_every_sample: the same nodes are listed, but none counts as copied.
        lasso (a Lasso): the mirror of simlod_query_lasso — rules L1-L4 on top of the planes; rule L5's promise is asserted likewise.  A lasso
        together with a footprint or a profile is a ValueError.
        return_index: the last element of the result is, per returned sample, its index in this export's samples (int64).
        invert: the mirror of simlod_query_inverse (include/simlod_hip.h, "inverse selections") — the classes the positive path computes,
        mapped by rule I2 (outside -> copied, copied -> emptied, filtered stays and takes the samples that FAIL the test); no node is left out
        of the walk (rule I3).  The F5 / L5 assertions stay as they are: an outside node holds no sample of the contract that passes, a copied
        node none that fails — the two facts the inverse relies on.  With a profile: ValueError."""
        if lasso is not None and (footprint is not None or profile is not None):
            raise ValueError("a lasso does not combine with a footprint or a profile in one call")
        if invert and profile is not None:
            raise ValueError("inverse profile queries are not covered")
        if self.select != abi.EXPORT_ALL or self.max_level < abi.MAX_DEPTH:
            raise ValueError(f"crop needs a full export (select all, max level 20), not select {self.select} / max level {self.max_level}")
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)
        if sel not in (abi.EXPORT_ALL, abi.EXPORT_CUT):
            raise ValueError("a region query selects 'all' or 'cut'")
        ml = abi.MAX_DEPTH if max_level is None else max(0, min(int(max_level), abi.MAX_DEPTH))
        src, smp = self.nodes, self.samples
        pl = np.asarray(region.planes, dtype=np.float32).astype(np.float64)
        mn, size = _box_of(self.box_min, self.box_max)
        outside, inside = classify_nodes(pl, src, self.box_min, self.box_max)
        if footprint is not None:
            # rule F4: outside by either, copied iff copied by both
            near, corner = classify_footprint(footprint, src, self.box_min, self.box_max)
            outside, inside = outside | (~near & ~corner), inside & ~near & corner
        if lasso is not None:
            # rule L4, combined as rule F4 combines: outside by either, copied iff copied by both
            behind, covered = classify_lasso(lasso, src, self.box_min, self.box_max)
            outside, inside = outside | behind, inside & covered
        if profile is not None:
            # rule P3, combined as rule F4 combines: outside by either, copied iff copied by both
            far, covered = classify_profile(profile, src, self.box_min, self.box_max)
            outside, inside = outside | far, inside & covered
        if test_every_sample:
            inside = np.zeros_like(inside)
        # the breadth-first walk over the listed nodes
        order, parent, masks, firsts = [0], [abi.EXPORT_NONE], [], []
        t = 0
        while t < len(order):
            nd = src[order[t]]
            mask, first = 0, abi.EXPORT_NONE
            if int(nd["level"]) < ml and nd["childMask"]:
                c = int(nd["firstChild"])
                for k in range(8):
                    if not (int(nd["childMask"]) >> k) & 1:
                        continue
                    if invert or not outside[c]:
                        if first == abi.EXPORT_NONE:
                            first = len(order)
                        mask |= 1 << k
                        order.append(c)
                        parent.append(t)
                    c += 1
            masks.append(mask)
            firsts.append(first)
            t += 1
        order = np.asarray(order, dtype=np.int64)
        out = src[order].copy()
        out["parent"], out["firstChild"], out["childMask"] = parent, firsts, masks
        leaf = (out["flags"] & abi.EXPORT_FLAG_LEAF) != 0
        chosen = np.ones(len(out), bool) if sel == abi.EXPORT_ALL else leaf | (out["level"] == ml)
        out["flags"] = np.where(leaf, abi.EXPORT_FLAG_LEAF, 0) | np.where(chosen, abi.EXPORT_FLAG_SELECTED, 0)
        # (inverse: the emptied nodes — the positive query's copied ones — contribute nothing, rule I4)
        cand = np.where(chosen & ~(inside if invert else outside)[order], src["numSamples"][order], 0).astype(np.int64)
        # rule 3 on every sample at once; rule 4's promise on the samples of the contract (finite, in the half-open box)
        x, y, z = (smp[a].astype(np.float64) for a in ("x", "y", "z"))
        ok = np.ones(len(smp), bool)
        with np.errstate(invalid="ignore"):
            for nx, ny, nz, d in pl:
                ok &= ((nx * x + ny * y) + nz * z) + d >= 0
            inbox = (x >= mn[0]) & (x < mn[0] + size) & (y >= mn[1]) & (y < mn[1] + size) & (z >= mn[2]) & (z < mn[2] + size)
        if profile is not None:
            ok &= profile.locate(smp)[0] >= 0
        if footprint is not None or profile is not None or lasso is not None:
            if footprint is not None:
                ok &= footprint.contains(smp)
            if lasso is not None:
                ok &= lasso.contains(smp)
            # rule F5 / P4 / L5 for every outside node of the source, listed or not: none of its samples of the contract passes (the copied ones below)
            bad = ok & inbox & np.repeat(outside, src["numSamples"].astype(np.int64))
            assert not bad.any(), f"node {int(np.repeat(np.arange(len(src)), src['numSamples'].astype(np.int64))[bad][0])} is outside and holds a sample of the box that passes the test"
        if invert:
            # the positive path's assertion for its copied nodes, which the inverse empties: none of their samples of the contract fails
            for i in np.nonzero(inside & (src["numSamples"] != 0))[0]:
                a = int(src["firstSample"][i])
                seg = slice(a, a + int(src["numSamples"][i]))
                assert (ok[seg] | ~inbox[seg]).all(), f"node {i} is copied and holds a sample of the box that fails the test"
        parts, ns_out = [], np.zeros(len(out), np.int64)
        n_filtered = n_copied = 0
        for t in np.nonzero(cand)[0]:
            i = order[t]
            a = int(src["firstSample"][i])
            seg = slice(a, a + int(cand[t]))
            if invert:
                if outside[i]:                                      # rule I2: every sample, no test
                    parts.append(np.arange(seg.start, seg.stop, dtype=np.int64))
                    n_copied += 1
                else:                                               # rule I1
                    parts.append(seg.start + np.nonzero(~ok[seg])[0].astype(np.int64))
                    n_filtered += 1
            elif inside[i]:
                assert (ok[seg] | ~inbox[seg]).all(), f"node {i} is copied and holds a sample of the box that fails the test"
                parts.append(np.arange(seg.start, seg.stop, dtype=np.int64))
                n_copied += 1
            else:
                parts.append(seg.start + np.nonzero(ok[seg])[0].astype(np.int64))
                n_filtered += 1
            ns_out[t] = len(parts[-1])
        out["numSamples"] = ns_out
        out["firstSample"] = np.concatenate([[0], np.cumsum(ns_out)[:-1]]).astype(np.uint64)
        index = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        samples = smp[index]
        ex = OctreeExport(out, samples, self.box_min, self.box_max, ml, abi.EXPORT_REGION)
        c = np.zeros((), dtype=abi.query_counts_dtype)
        c["numNodes"], c["numSamples"], c["numCandidates"] = len(out), len(samples), int(cand.sum())
        c["numFilteredNodes"], c["numCopiedNodes"] = n_filtered, n_copied
        got = (ex, c) if return_counts else (ex,)
        if return_index:
            got += (index,)
        return got if len(got) > 1 else ex

    # -- paint regions (include/simlod_hip.h, "paint regions") -----------------------------------------------------------------------------
    def paint(self, region, paint, footprint=None, colors=None, return_previous=False, lasso=None, invert=False):
        """The host mirror of simlod_paint_region on the octree this FULL export was taken from: (this export with the colours of the target
        samples changed — a new OctreeExport on the host; table, positions and order are this one's —, the SimlodQueryCounts record) and,
        return_previous, the colour words those samples had, in the query's order (uint32).  The target set and its order are crop's (rule
        E0: max level 20, select "all"), so rule F5's assertion stays in force.  colors: the uint32 words of an ARRAY paint, one per target
        sample at least.  lasso (a Lasso, no footprint then): the mirror of simlod_paint_lasso, the target set being crop(lasso=)'s.
        invert: the mirror of simlod_paint_inverse, the target set being crop(invert=True)'s (rule I8)."""
        _, c, index = self.crop(region, abi.MAX_DEPTH, "all", return_counts=True, footprint=footprint, return_index=True, lasso=lasso, invert=invert)
        smp = self.samples.copy()
        previous = smp["color"][index].copy()
        if paint.mode == abi.PAINT_ARRAY:
            if colors is None:
                raise ValueError("an ARRAY paint needs colors")
            colors = np.asarray(colors, dtype=np.uint32).reshape(-1)
            if len(colors) < len(index):
                raise ValueError(f"{len(colors)} colours for {len(index)} samples")
            new = colors[: len(index)]
        else:
            new = paint.apply(previous, smp["z"][index])
        smp["color"][index] = new
        ex = OctreeExport(self.nodes.copy(), smp, self.box_min, self.box_max, self.max_level, self.select)
        return (ex, c, previous) if return_previous else (ex, c)

    # -- summary queries (include/simlod_hip.h, "summary queries") -------------------------------------------------------------------------
    def summarize(self, region, max_level=None, select="cut", footprint=None, z0=0.0, scale=1.0, return_counts=False, lasso=None, invert=False):
        """The host mirror of simlod_query_summary on the octree this FULL export was taken from: the Summary of the samples
        crop(region, max_level, select, footprint=footprint) returns (rule S0: the set is crop's by construction) — and, return_counts, the
        SimlodQueryCounts record too.  Rules S1-S4 in numpy float64 and unsigned integers, in the order the header gives; the z histogram's
        index is Paint.ramp_index (rule E3) with z0 and scale as float32.  lasso (a Lasso, no footprint then): the mirror of
        simlod_query_summary_lasso, the set being crop(lasso=)'s.  invert: the mirror of simlod_query_summary_inverse, the set being
        crop(invert=True)'s (rule I8)."""
        bins = Paint(abi.PAINT_RAMP, z0=z0, scale=scale)                    # (refuses what rule S8 refuses of z0 and scale)
        ex, c = self.crop(Region() if region is None else region, max_level, select, return_counts=True, footprint=footprint, lasso=lasso, invert=invert)
        smp = ex.samples
        mn, size = _box_of(self.box_min, self.box_max)
        rec = np.zeros((), dtype=abi.summary_dtype)
        rec["numSamples"] = len(smp)
        bits = [np.ascontiguousarray(smp[a]).view(np.uint32) for a in ("x", "y", "z")]
        finite = np.ones(len(smp), bool)
        inv = np.float64(abi.SUMMARY_CELLS) / size                          # rule S2: one IEEE division
        c16 = []
        for k, b in enumerate(bits):
            finite &= (b & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
            # rule S1: the key's order over the coordinates that are no NaN
            key = (b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))).astype(np.uint32)
            key = key[(b & np.uint32(0x7FFFFFFF)) <= np.uint32(0x7F800000)]
            lo, hi = (int(key.min()), int(key.max())) if len(key) else (0xFF800000, 0x007FFFFF)
            unkey = lambda v: v ^ (0x80000000 if v >> 31 else 0xFFFFFFFF)
            rec["min"][k], rec["max"][k] = np.array([unkey(lo), unkey(hi)], np.uint32).view(np.float32)
            # rule S2: the 20-bit cell, a NaN in cell 0
            c20 = cell20(b.view(np.float32), mn[k], inv)
            rec["sum"][k] = c20.sum(dtype=np.uint64)
            c16.append(c20 >> np.uint64(4))
        for j, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            rec["sum2"][j] = (c16[a] * c16[b]).sum(dtype=np.uint64)
        rec["numNonFinite"] = int((~finite).sum())
        rec["histZ"] = np.bincount(bins.ramp_index(smp["z"]), minlength=256).astype(np.uint64)
        for k in range(4):
            rec["histC"][k] = np.bincount((smp["color"] >> np.uint32(8 * k)) & np.uint32(255), minlength=256).astype(np.uint64)
        out = Summary(rec, bins.z0, bins.scale)
        return (out, c) if return_counts else out

    # -- compare queries (include/simlod_hip.h, "compare queries") -------------------------------------------------------------------------
    def compare(self, other, compare, count_only=False):
        """The host mirror of simlod_compare_samples on this export's samples (A) and `other`'s (B; may be this export), in this export's box:
        compare_samples' (records, colours, summary)."""
        return compare_samples(self.samples, other.samples, (self.box_min, self.box_max), compare, count_only=count_only)

    # -- cluster queries (include/simlod_hip.h, "cluster queries") -------------------------------------------------------------------------
    def cluster(self, cluster, count_only=False):
        """The host mirror of simlod_cluster_samples on this export's samples, in this export's box: cluster_samples' (records, colours,
        summary)."""
        return cluster_samples(self.samples, (self.box_min, self.box_max), cluster, count_only=count_only)

    # -- surface queries (include/simlod_hip.h, "surface queries") -------------------------------------------------------------------------
    def surface(self, surface, other=None, count_only=False):
        """The host mirror of simlod_surface_samples on this export's samples (A) and `other`'s (B; None: this export), in this export's box:
        surface_samples' (records, colours, summary)."""
        other = self if other is None else other
        return surface_samples(self.samples, other.samples, (self.box_min, self.box_max), surface, count_only=count_only)

    # -- profile queries (include/simlod_hip.h, "profile queries") -------------------------------------------------------------------------
    def profile(self, profile, region=None, max_level=None, select="all", return_counts=False, test_every_sample=False):
        """The host mirror of simlod_query_profile on the octree this FULL export was taken from: (the samples in the corridor as an OctreeExport
        on the host, their records as an array of abi.profile_sample_dtype) — and, return_counts, the SimlodQueryCounts record too.  Rule P4 is
        asserted for every copied and every outside node (crop).  test_every_sample: rule P3 prunes the table as it does, but no node is copied
        without a test; by rule P4 the samples and records are the same."""
        got = self.crop(Region() if region is None else region, max_level, select, return_counts, profile=profile, test_every_sample=test_every_sample)
        ex = got[0] if return_counts else got
        records = profile.records(ex.samples)
        return (ex, records, got[1]) if return_counts else (ex, records)

    # -- view queries (include/simlod_hip.h, "view queries") ---------------------------------------------------------------------------------
    def view(self, uniforms, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None, return_counts=False):
        """The host mirror of simlod_query_view on the octree this FULL export was taken from: what the device returns for the camera of
        `uniforms`, as an OctreeExport on the host (select "visible") — and, return_counts, the SimlodViewCounts record too, with the ladder
        samplesAt.  numpy float32 throughout (view_geometry).  When no bias in [bias, max_bias] fits `budget`: ValueError — or,
        return_counts, the table of max_bias without samples and counts whose error has abi.EXPORT_ERR_BUDGET, as the device leaves them."""
        if not 0 <= int(bias) <= int(max_bias) <= abi.VIEW_MAX_BIAS:
            raise ValueError("0 <= bias <= max_bias <= 20")
        full = self.truncated(max_level, "all")                   # rule V1: the listed nodes, every one with its count
        out, smp = full.nodes.copy(), full.samples
        inside, _, _, rank = view_geometry(uniforms, out)
        ns = out["numSamples"].astype(np.int64)
        leaf = (out["flags"] & abi.EXPORT_FLAG_LEAF) != 0
        visible = (inside | (not cull)) & (ns > 0)
        par = out["parent"].astype(np.int64)
        P = np.where(par == abi.EXPORT_NONE, abi.VIEW_MAX_BIAS + 1 if draw_small_root else 0, rank[np.where(par == abi.EXPORT_NONE, 0, par)])
        b = np.arange(abi.VIEW_MAX_BIAS + 1)[:, None]
        drawn = visible[None, :] & np.where(b < rank[None, :], leaf[None, :], b < P[None, :])            # rule V4, bias by node
        ladder = (drawn * ns[None, :]).sum(axis=1)
        limit = abi.VIEW_NO_BUDGET if budget is None else int(budget)
        fits = [k for k in range(int(bias), int(max_bias) + 1) if int(ladder[k]) <= limit]
        chosen = fits[0] if fits else int(max_bias)
        if not fits and not return_counts:
            raise ValueError(f"no bias in [{int(bias)}, {int(max_bias)}] fits {limit} samples (the coarsest holds {int(ladder[chosen])})")
        sel = drawn[chosen]
        out["flags"] = np.where(leaf, abi.EXPORT_FLAG_LEAF, 0) | np.where(sel, abi.EXPORT_FLAG_SELECTED, 0)
        out["numSamples"] = np.where(sel, ns, 0)
        out["firstSample"] = np.concatenate([[0], np.cumsum(np.where(sel, ns, 0))[:-1]]).astype(np.uint64)
        samples = smp[np.repeat(sel, ns)] if fits else np.zeros(0, dtype=abi.point_dtype)
        ex = OctreeExport(out, samples, self.box_min, self.box_max, full.max_level, abi.EXPORT_VISIBLE)
        if not return_counts:
            return ex
        c = np.zeros((), dtype=abi.view_counts_dtype)
        c["numNodes"], c["error"], c["numSamples"] = len(out), 0 if fits else abi.EXPORT_ERR_BUDGET, int(ladder[chosen])
        c["bias"], c["numSelected"], c["numInside"], c["samplesAt"] = chosen, int(sel.sum()), int(visible.sum()), ladder
        return ex, c

    # -- view deltas (include/simlod_hip.h, "view deltas") ---------------------------------------------------------------------------------
    def view_delta(self, uniforms, held, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None, tails=False):
        """The host mirror of simlod_query_view_delta on the octree this FULL export was taken from: `view` with the same arguments, and what
        of its cut a receiver that holds `held` (an OctreeExport, or None: nothing) lacks — a ViewDelta on the host, whose counts are the
        SimlodDeltaCounts record.  When no bias fits the budget the delta is empty and counts["view"]["error"] has abi.EXPORT_ERR_BUDGET."""
        new, vc = self.view(uniforms, bias, max_bias, budget, cull, draw_small_root, max_level, return_counts=True)
        return delta_between(new, held, tails, vc)

    # -- ray queries (include/simlod_hip.h, "ray queries") -----------------------------------------------------------------------------------
    def truncated(self, max_level=None, select="cut"):
        """What simlod_export_octree(max_level, select) writes for the octree this FULL export was taken from ("all" or "cut"): breadth-first
        order keeps the levels together, so the table is a prefix of this one with the entries at max_level cut off from their children."""
        if self.select != abi.EXPORT_ALL or self.max_level < abi.MAX_DEPTH:
            raise ValueError(f"needs a full export (select all, max level 20), not select {self.select} / max level {self.max_level}")
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)
        if sel not in (abi.EXPORT_ALL, abi.EXPORT_CUT):
            raise ValueError("only 'all' and 'cut' follow from a full export")
        ml = abi.MAX_DEPTH if max_level is None else max(0, min(int(max_level), abi.MAX_DEPTH))
        src, smp = self.nodes, self.samples
        k = int((src["level"] <= ml).sum())
        out = src[:k].copy()
        assert (out["level"] <= ml).all(), "the table is not in breadth-first order"
        cut = out["level"] == ml
        out["childMask"][cut], out["firstChild"][cut] = 0, abi.EXPORT_NONE
        leaf = (out["flags"] & abi.EXPORT_FLAG_LEAF) != 0
        chosen = np.ones(k, bool) if sel == abi.EXPORT_ALL else leaf | cut
        out["flags"] = np.where(leaf, abi.EXPORT_FLAG_LEAF, 0) | np.where(chosen, abi.EXPORT_FLAG_SELECTED, 0)
        ns = src["numSamples"][:k].astype(np.int64)
        out["numSamples"] = np.where(chosen, ns, 0)
        out["firstSample"] = np.concatenate([[0], np.cumsum(out["numSamples"].astype(np.int64))[:-1]]).astype(np.uint64)
        samples = smp[: int(ns.sum())][np.repeat(chosen, ns)]
        return OctreeExport(out, samples, self.box_min, self.box_max, ml, sel)

    def cast(self, rays, max_level=None, select="cut", return_counts=False, return_passing=False):
        """The host mirror of simlod_query_rays on the octree this FULL export was taken from: the hits (abi.ray_hit_dtype, one per ray) whose
        `node` / `ordinal` index the table and sample ranges of export_octree(max_level, select) — and, return_counts, the SimlodRayCounts
        record; return_passing, the number of samples of its pairs that pass the test, per ray."""
        return self.truncated(max_level, select).cast_selected(rays, return_counts, return_passing)

    def _ray_pairs(self, rec):
        """Rules 1 and 3 for SimlodRay records against this table: (valid per ray, [(table index, the rays paired with it)] in table order)."""
        o, d = rec["origin"].astype(np.float64), rec["dir"].astype(np.float64)
        tmin, tmax, rad, spr = (rec[f].astype(np.float64) for f in ("tMin", "tMax", "radius", "spread"))
        with np.errstate(invalid="ignore", over="ignore"):
            valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(tmin) & np.isfinite(tmax) & np.isfinite(rad) & np.isfinite(spr)
            valid &= (d != 0).any(1) & (tmin >= 0) & (tmin <= tmax) & (rad >= 0) & (spr >= 0) & (rec["reserved"] == 0).all(1)
            R = rad + spr * tmax
        return valid, self._descend(valid, lambda lo, hi, idx: _slab(lo, hi, o[idx], d[idx], tmin[idx], tmax[idx], R[idx]))

    def _descend(self, valid, probe):
        """The table descent the ray and the neighbour mirror share: probe(lo, hi, idx) says which of the probes `idx` pass the node's inflated
        cube [lo, hi]; a probe reaches a node iff it passed every listed ancestor.  -> [(table index, the probes paired with it)] in table
        order, for the selected entries with samples."""
        tb = self.nodes
        mn, size = _box_of(self.box_min, self.box_max)
        e = np.ldexp(size, -abi.MAX_DEPTH)
        reach = {0: np.nonzero(valid)[0]}
        pairs = []
        for t in range(len(tb)):
            idx = reach.pop(t, None)
            if idx is None or len(idx) == 0:
                continue
            nd = tb[t]
            s = np.ldexp(size, -int(nd["level"]))
            A = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=np.float64)
            lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e
            idx = idx[probe(lo, hi, idx)]
            if len(idx) == 0:
                continue
            c = int(nd["firstChild"])
            for k in range(8):
                if (int(nd["childMask"]) >> k) & 1:
                    reach[c] = idx
                    c += 1
            if int(nd["numSamples"]) != 0 and int(nd["flags"]) & abi.EXPORT_FLAG_SELECTED:
                pairs.append((t, idx))
        return pairs

    def _per_node(self, pairs):
        out = np.zeros(self.num_nodes, np.int64)
        for t, idx in pairs:
            out[t] = len(idx)
        return out

    def _pair_blocks(self, pairs, totals):
        """The loop the ray and the neighbour mirror share, per pair list of _descend (nodes in ascending order): yields (table index, the
        node's first sample, its sample slice, a block of at most 2^21 // numSamples of its probes); totals[0] += pairs, totals[1] +=
        candidates on the way."""
        tb = self.nodes
        for t, idx in pairs:
            ns, a = int(tb["numSamples"][t]), int(tb["firstSample"][t])
            totals[0] += len(idx)
            totals[1] += len(idx) * ns
            step = max(1, (1 << 21) // ns)
            for b in range(0, len(idx), step):
                yield t, a, slice(a, a + ns), idx[b:b + step]

    def rays_per_node(self, rays):
        """How many rays form a pair with each table entry (rule 3 alone: no sample is tested)."""
        return self._per_node(self._ray_pairs(_ray_records(rays))[1])

    def cast_selected(self, rays, return_counts=False, return_passing=False):
        """The mirror on an export whose selection is already made (any `select`, "visible" included): the nodes considered are this table's."""
        rec = _ray_records(rays)
        tb, smp = self.nodes, self.samples
        n = len(rec)
        hits = np.zeros(n, dtype=abi.ray_hit_dtype)
        hits["t"], hits["node"], hits["ordinal"] = np.inf, abi.EXPORT_NONE, abi.EXPORT_NONE
        passing = np.zeros(n, np.int64)
        o, d = rec["origin"].astype(np.float64), rec["dir"].astype(np.float64)
        tmin, tmax, rad, spr = (rec[f].astype(np.float64) for f in ("tMin", "tMax", "radius", "spread"))
        with np.errstate(invalid="ignore", over="ignore"):
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        x, y, z = (smp[a].astype(np.float64) for a in ("x", "y", "z"))
        valid, pairs = self._ray_pairs(rec)
        totals = [0, 0]
        for t, a, sl, i in self._pair_blocks(pairs, totals):
            sx, sy, sz = x[sl], y[sl], z[sl]
            col = lambda v: v[i][:, None]
            dx, dy, dz = col(d[:, 0]), col(d[:, 1]), col(d[:, 2])
            with np.errstate(invalid="ignore", over="ignore"):
                px, py, pz = sx[None, :] - col(o[:, 0]), sy[None, :] - col(o[:, 1]), sz[None, :] - col(o[:, 2])
                tt = ((dx * px + dy * py) + dz * pz) / col(dd)
                qx, qy, qz = px - tt * dx, py - tt * dy, pz - tt * dz
                s2 = (qx * qx + qy * qy) + qz * qz
                rr = col(rad) + col(spr) * tt
                ok = (tt >= col(tmin)) & (tt <= col(tmax)) & (s2 <= rr * rr)
            passing[i] += ok.sum(1)
            tm = np.where(ok, tt, np.inf)
            j = tm.argmin(1)                                   # (the first of equal minima: the smallest ordinal)
            tb_ = tm[np.arange(len(i)), j]
            upd = tb_ < hits["t"][i]                           # (nodes in ascending order: an equal t keeps the smaller node)
            iu, ju = i[upd], j[upd]
            hits["t"][iu], hits["node"][iu], hits["ordinal"][iu] = tb_[upd], t, ju
            hits["sample"][iu] = smp[a + ju]
        out = [hits]
        if return_counts:
            c = np.zeros((), dtype=abi.ray_counts_dtype)
            c["numNodes"], c["numHits"], c["numInvalid"] = len(tb), int((hits["node"] != abi.EXPORT_NONE).sum()), int((~valid).sum())
            c["numPairs"], c["numCandidates"] = totals
            out.append(c)
        if return_passing:
            out.append(passing)
        return out[0] if len(out) == 1 else tuple(out)

    # -- neighbour queries (include/simlod_hip.h, "neighbour queries") -----------------------------------------------------------------------
    def neighbours(self, spheres, k, max_level=None, select="cut", return_counts=False):
        """The host mirror of simlod_query_neighbours on the octree this FULL export was taken from: (the neighbours as an (n, k) array of
        abi.neighbour_dtype whose `node` / `ordinal` index the table and sample ranges of export_octree(max_level, select), `within` per
        query) — and, return_counts, the SimlodNeighbourCounts record."""
        return self.truncated(max_level, select).neighbours_selected(spheres, k, return_counts)

    def _sphere_pairs(self, rec):
        """Rules 1 and 3 for SimlodSphere records against this table: (valid per query, [(table index, the queries paired with it)] in table order)."""
        c, r = rec["center"].astype(np.float64), rec["radius"].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            valid = np.isfinite(c).all(1) & np.isfinite(r) & (r >= 0)
            rr = r * r

        def probe(lo, hi, idx):
            with np.errstate(invalid="ignore", over="ignore"):
                ex = np.maximum(np.maximum(lo - c[idx], 0.0), c[idx] - hi)
                return (ex[:, 0] * ex[:, 0] + ex[:, 1] * ex[:, 1]) + ex[:, 2] * ex[:, 2] <= rr[idx]
        return valid, self._descend(valid, probe)

    def spheres_per_node(self, spheres):
        """How many queries form a pair with each table entry (rule 3 alone: no sample is tested)."""
        return self._per_node(self._sphere_pairs(_sphere_records(spheres))[1])

    def neighbours_selected(self, spheres, k, return_counts=False):
        """The mirror on an export whose selection is already made (any `select`, "visible" included): the nodes considered are this table's."""
        k = int(k)
        if not 1 <= k <= abi.NEIGHBOURS_MAX_K:
            raise ValueError(f"k = {k}: 1 .. {abi.NEIGHBOURS_MAX_K}")
        rec = _sphere_records(spheres)
        tb, smp = self.nodes, self.samples
        n = len(rec)
        best = np.zeros((n, k), dtype=abi.neighbour_dtype)
        best["d2"], best["node"], best["ordinal"] = np.inf, abi.EXPORT_NONE, abi.EXPORT_NONE
        within = np.zeros(n, np.int64)
        c, r = rec["center"].astype(np.float64), rec["radius"].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            rr = r * r
        x, y, z = (smp[a].astype(np.float64) for a in ("x", "y", "z"))
        valid, pairs = self._sphere_pairs(rec)
        totals = [0, 0]
        for t, a, sl, i in self._pair_blocks(pairs, totals):
            sx, sy, sz = x[sl], y[sl], z[sl]
            with np.errstate(invalid="ignore", over="ignore"):
                px, py, pz = sx[None, :] - c[i, 0][:, None], sy[None, :] - c[i, 1][:, None], sz[None, :] - c[i, 2][:, None]
                d2 = (px * px + py * py) + pz * pz
                ok = d2 <= rr[i][:, None]
            within[i] += ok.sum(1)
            cols = np.nonzero(ok.any(0))[0]                    # (ascending ordinals: the stable sort below keeps the smaller one first)
            if len(cols) == 0:
                continue
            sub = np.where(ok[:, cols], d2[:, cols], np.inf)
            order = np.argsort(sub, axis=1, kind="stable")[:, :k]
            new = np.zeros((len(i), order.shape[1]), dtype=abi.neighbour_dtype)
            new["d2"] = np.take_along_axis(sub, order, 1)
            hit = np.isfinite(new["d2"])
            new["node"], new["ordinal"] = np.where(hit, t, abi.EXPORT_NONE), np.where(hit, cols[order], abi.EXPORT_NONE)
            new["sample"][hit] = smp[a + cols[order]][hit]
            # what was found so far comes from smaller nodes: a stable sort by d2 keeps the total order (d2, node, ordinal)
            both = np.concatenate([best[i], new], axis=1)
            keep = np.argsort(both["d2"], axis=1, kind="stable")[:, :k]
            best[i] = np.take_along_axis(both, keep, 1)
        if not return_counts:
            return best, within
        cn = np.zeros((), dtype=abi.neighbour_counts_dtype)
        cn["numNodes"], cn["numInvalid"], cn["k"] = len(tb), int((~valid).sum()), k
        cn["numPairs"], cn["numCandidates"] = totals
        cn["numFound"], cn["numWithin"] = int(np.minimum(within, k).sum()), int(within.sum())
        return best, within, cn

    def save(self, path):
        h = np.zeros(1, dtype=header_dtype)
        h["magic"], h["version"], h["select"], h["max_level"], h["header_bytes"] = MAGIC, VERSION, self.select, self.max_level, HEADER_BYTES
        h["numNodes"], h["numSamples"] = self.num_nodes, self.num_samples
        h["box_min"], h["box_max"] = self.box_min, self.box_max
        with open(path, "wb") as f:
            f.write(h.tobytes())
            f.write(self.table_tensor.cpu().numpy().tobytes())
            f.write(self.samples_tensor.cpu().numpy().tobytes())

    @classmethod
    def load(cls, path):
        """Read a file written by save(); the table is validated before the export is returned (host tensors)."""
        raw = np.fromfile(path, dtype=np.uint8)
        if raw.size < HEADER_BYTES:
            raise ValueError(f"{path}: truncated header")
        h = raw[:HEADER_BYTES].view(header_dtype)[0]
        if bytes(h["magic"]).ljust(8, b"\0") != MAGIC:
            raise ValueError(f"{path}: not an octree export (magic)")
        if int(h["version"]) != VERSION or int(h["header_bytes"]) != HEADER_BYTES:
            raise ValueError(f"{path}: unsupported version {int(h['version'])}")
        if int(h["select"]) > abi.EXPORT_REGION:
            raise ValueError(f"{path}: unknown selection {int(h['select'])}")
        n, m = int(h["numNodes"]), int(h["numSamples"])
        tb, sb = n * abi.export_node_dtype.itemsize, m * abi.point_dtype.itemsize
        if raw.size != HEADER_BYTES + tb + sb:
            raise ValueError(f"{path}: {raw.size} bytes, the header announces {HEADER_BYTES + tb + sb}")
        ex = cls(raw[HEADER_BYTES: HEADER_BYTES + tb].copy(), raw[HEADER_BYTES + tb:].copy(), h["box_min"], h["box_max"], int(h["max_level"]), int(h["select"]))
        return ex.validate()

    def pack(self, return_counts=False):
        """The same export with 8-byte samples (rules K0-K7 of "packed samples", in numpy): a PackedExport on the host, and with return_counts
        the SimlodPackCounts record.  DeviceOctree.pack does the same on the device."""
        packed, c = pack_samples(self.nodes, self.samples, self.box_min, self.box_max)
        px = PackedExport(self.nodes, packed, self.box_min, self.box_max, self.max_level, self.select)
        return (px, c) if return_counts else px


def cell20(x, box_min, inv):
    """Summary rule S2's 20-bit cell of float32 coordinates on an axis whose box starts at box_min, as uint64 (summary_rules.hpp
    summary_cell20): t = ((double)x - (double)boxMin) * inv; 1048575 if t >= 1048575.0, (uint32_t)t if t > 0.0, else 0 (a NaN gives 0).  The
    summary's mirror passes rule S2's inv, the compare mirror rule C4's: the one statement both rules rest on."""
    top = np.float64(abi.SUMMARY_CELLS - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float32).astype(np.float64) - np.float64(box_min)) * np.float64(inv)
        return np.where(t >= top, top, np.where(t > 0.0, t, 0.0)).astype(np.uint64)


def cell20_f64(x, box_min, inv):
    """cell20 for float64 coordinates (align_rules.hpp align_cell20, rule A2): the same clamp on t = (x - boxMin) * inv."""
    top = np.float64(abi.SUMMARY_CELLS - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float64) - np.float64(box_min)) * np.float64(inv)
        return np.where(t >= top, top, np.where(t > 0.0, t, 0.0)).astype(np.uint64)


def _box_of(box_min, box_max):
    """(min as float64, size): the box as construct.hip derives it — the largest of the fp32 differences boxMax - boxMin."""
    mn32, mx32 = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    return mn32.astype(np.float64), np.float64((mx32 - mn32).max())


def classify_nodes(planes, nodes, box_min, box_max):
    """Rules 1 and 4 of the region query for every entry of a table: (outside, inside) as boolean arrays — the inflated cube of the node
    against every plane (N x 4, float64 values of the float32 coefficients).  Neither: the node is filtered sample by sample."""
    mn, size = _box_of(box_min, box_max)
    s = np.ldexp(size, -nodes["level"].astype(np.int64))[:, None]
    e = np.ldexp(size, -abi.MAX_DEPTH)
    A = np.stack([nodes["X"], nodes["Y"], nodes["Z"]], axis=1).astype(np.float64)
    lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e
    outside, inside = np.zeros(len(nodes), bool), np.ones(len(nodes), bool)
    for nx, ny, nz, d in np.asarray(planes, dtype=np.float64).reshape(-1, 4):
        fx, fy, fz = (hi if nx >= 0 else lo)[:, 0], (hi if ny >= 0 else lo)[:, 1], (hi if nz >= 0 else lo)[:, 2]
        gx, gy, gz = (lo if nx >= 0 else hi)[:, 0], (lo if ny >= 0 else hi)[:, 1], (lo if nz >= 0 else hi)[:, 2]
        outside |= ((nx * fx + ny * fy) + nz * fz) + d < 0
        inside &= ((nx * gx + ny * gy) + nz * gz) + d >= 0
    return outside, inside


def view_planes(transform):
    """The six frustum planes of a view query (include/simlod_hip.h, "view queries": planes) from the 4 x 4 matrix, normalised: 6 x 4 float32."""
    r = np.asarray(transform, dtype=np.float32).reshape(4, 4)
    with np.errstate(all="ignore"):
        P = np.stack([r[3] - r[0], r[3] + r[0], r[3] + r[1], r[3] - r[1], r[3] - r[2], r[3] + r[2]])
        d2 = P[:, 0] * P[:, 0]
        d2 = d2 + P[:, 1] * P[:, 1]
        d2 = d2 + P[:, 2] * P[:, 2]
        return P / np.sqrt(d2)[:, None]


def view_geometry(uniforms, nodes):
    """Rules V2 and V3 of the view query for every entry of a table (or any records with level, X, Y, Z) under the camera of `uniforms`:
    (inside, dx, dy, rank) — does the node's cube meet the frustum of transform_updateBound, the float32 extents of its screen box, and R,
    the number of biases 0..20 at which it is large.  numpy float32 in the header's operation order; fmin / fmax drop a NaN as fminf / fmaxf do."""
    f = np.float32
    u = np.asarray(uniforms).reshape(-1)[0]
    M = np.asarray(u["transform_updateBound"], dtype=f).reshape(4, 4)
    mn3, mx3 = np.asarray(u["boxMin"], dtype=f).reshape(3), np.asarray(u["boxMax"], dtype=f).reshape(3)
    width, height = f(u["width"]), f(u["height"])
    with np.errstate(all="ignore"):
        planes = view_planes(M)
        ext = mx3 - mn3
        size = np.fmax(np.fmax(ext[0], ext[1]), ext[2])
        s = (size / np.ldexp(f(1.0), nodes["level"].astype(np.int32))).astype(f)
        A = [nodes[a].astype(f) for a in ("X", "Y", "Z")]
        lo = [mn3[k] + (A[k] + f(0.0)) * s for k in range(3)]
        hi = [mn3[k] + (A[k] + f(1.0)) * s for k in range(3)]
        inside = np.ones(len(s), bool)
        for nx, ny, nz, c in planes:
            d = nx * (hi[0] if nx > 0 else lo[0])
            d = d + ny * (hi[1] if ny > 0 else lo[1])
            d = d + nz * (hi[2] if nz > 0 else lo[2])
            d = d + c
            inside &= ~(d < 0)

        def dot(r, x, y, z):
            t = r[0] * x
            t = t + r[1] * y
            t = t + r[2] * z
            return t + r[3] * f(1.0)

        sx, sy = [], []
        for k in range(8):                      # p000, p001, p010, p011, p100, p101, p110, p111
            x, y, z = (hi if k & 4 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 1 else lo)[2]
            cw = dot(M[3], x, y, z)
            sx.append(((dot(M[0], x, y, z) / cw) * f(0.5) + f(0.5)) * width)
            sy.append(((dot(M[1], x, y, z) / cw) * f(0.5) + f(0.5)) * height)

        def tree(op, v):
            return op(op(op(v[0], v[1]), op(v[2], v[3])), op(op(v[4], v[5]), op(v[6], v[7])))

        dx, dy = tree(np.fmax, sx) - tree(np.fmin, sx), tree(np.fmax, sy) - tree(np.fmin, sy)
        assert dx.dtype == f and dy.dtype == f and s.dtype == f
        lim = 2.0 * np.float64(f(u["minNodeSize"]))
        rank = np.zeros(len(s), np.int64)
        for b in range(abi.VIEW_MAX_BIAS + 1):
            lb = np.ldexp(lim, b)
            rank += (dx.astype(np.float64) > lb) | (dy.astype(np.float64) > lb)
    return inside, dx, dy, rank


def delta_keys(nodes):
    """The order of a table's entries as keys: (level, Morton(X, Y, Z)) per entry, the Morton code as uint64 with bit i of X at 3 i + 2, of Y at
    3 i + 1, of Z at 3 i (delta_rules.hpp delta_key)."""
    m = np.zeros(len(nodes), np.uint64)
    for i in range(21):
        for a, sh in (("X", 2), ("Y", 1), ("Z", 0)):
            m |= ((nodes[a].astype(np.uint64) >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + sh)
    return nodes["level"].astype(np.int64), m


def delta_find(held, nodes):
    """Rule D2 for every entry of `nodes`: the index of the held entry with its (level, X, Y, Z), else abi.EXPORT_NONE — by the device's search
    (delta_rules.hpp delta_find: the first held entry whose key is not below the wanted one, then the four words compared), so that a held
    table that is not in key order misses what the device misses."""
    n, nh = len(nodes), len(held)
    out = np.full(n, abi.EXPORT_NONE, np.int64)
    if n == 0 or nh == 0:
        return out
    hl, hm = delta_keys(held)
    wl, wm = delta_keys(nodes)
    lo, hi = np.zeros(n, np.int64), np.full(n, nh, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = np.where(act, lo + ((hi - lo) >> 1), 0)
        less = (hl[mid] < wl) | ((hl[mid] == wl) & (hm[mid] < wm))
        lo = np.where(act & less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)
    at = np.minimum(lo, nh - 1)
    same = (lo < nh) & (held["level"][at] == nodes["level"]) & (held["X"][at] == nodes["X"]) & (held["Y"][at] == nodes["Y"]) & (held["Z"][at] == nodes["Z"])
    out[same] = lo[same]
    return out


def delta_between(new, held, tails=False, view_counts=None):
    """Rules D2-D6 between a cut `new` (an OctreeExport as `view` returns it) and a held table (an OctreeExport or None) -> a ViewDelta on the
    host.  view_counts: the SimlodViewCounts record that goes with `new` (None: one with numNodes, numSamples and numSelected alone); with
    abi.EXPORT_ERR_BUDGET in its error every entry has state NONE (rule D1)."""
    tb, smp = new.nodes, new.samples
    ht = held.nodes if held is not None else np.zeros(0, dtype=abi.export_node_dtype)
    n = len(tb)
    budget_error = view_counts is not None and bool(int(view_counts["error"]) & abi.EXPORT_ERR_BUDGET)
    h = delta_find(ht, tb)
    found = h != abi.EXPORT_NONE
    hh = np.where(found, h, 0)
    hflags = ht["flags"][hh] if len(ht) else np.zeros(n, np.uint8)
    hns = ht["numSamples"][hh].astype(np.int64) if len(ht) else np.zeros(n, np.int64)
    ns = tb["numSamples"].astype(np.int64)
    selected = (tb["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
    hs = np.where(found & ((hflags & abi.EXPORT_FLAG_SELECTED) != 0), hns, 0)
    kind = found & (((tb["flags"] ^ hflags) & abi.EXPORT_FLAG_LEAF) == 0)
    kept = selected & kind & (hs == ns) & (ns > 0)
    grown = selected & ~kept & bool(tails) & kind & (hs > 0) & (hs < ns)
    state = np.where(kept, abi.DELTA_KEPT, np.where(grown, abi.DELTA_GROWN, np.where(selected, abi.DELTA_ADDED, abi.DELTA_NONE)))
    num_kept = np.where(kept, ns, np.where(grown, hs, 0))
    num_delta = ns - num_kept
    if budget_error:
        state[:], num_kept[:], num_delta[:] = abi.DELTA_NONE, 0, 0
    entries = np.zeros(n, dtype=abi.delta_entry_dtype)
    entries["held"], entries["state"], entries["numKept"], entries["numDelta"] = h, state, num_kept, num_delta
    entries["firstDelta"] = np.concatenate([[0], np.cumsum(num_delta)[:-1]]).astype(np.uint64) if n else 0
    parts = []
    if not budget_error:
        for t in np.nonzero(num_delta)[0]:
            a = int(tb["firstSample"][t])
            parts.append(smp[a + int(num_kept[t]): a + int(ns[t])])
    delta = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)
    # rule D6
    taken = np.zeros(len(ht), bool)
    taken[h[(state == abi.DELTA_KEPT) | (state == abi.DELTA_GROWN)]] = True
    dropped = np.nonzero(((ht["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (ht["numSamples"] > 0) & ~taken)[0].astype(np.uint32)
    c = np.zeros((), dtype=abi.delta_counts_dtype)
    if view_counts is not None:
        c["view"] = view_counts
    else:
        c["view"]["numNodes"], c["view"]["numSamples"], c["view"]["numSelected"] = n, int(ns.sum()), int(selected.sum())
    c["numDeltaSamples"], c["numKeptSamples"] = int(num_delta.sum()), int(num_kept.sum())
    c["numKept"], c["numGrown"], c["numAdded"] = int((state == abi.DELTA_KEPT).sum()), int((state == abi.DELTA_GROWN).sum()), int((state == abi.DELTA_ADDED).sum())
    c["numDropped"] = len(dropped)
    return ViewDelta(tb, entries, delta, dropped, new.box_min, new.box_max, new.max_level, c)


class ViewDelta:
    """What simlod_query_view_delta returns (include/simlod_hip.h, "view deltas"): the new cut's table (abi.export_node_dtype), one
    abi.delta_entry_dtype record per table entry, the delta samples (abi.point_dtype), the held indices to drop (uint32), each as a uint8
    tensor on the host or on a device, with the box, max_level and the SimlodDeltaCounts record (host)."""

    def __init__(self, table, entries, samples, dropped, box_min, box_max, max_level=20, counts=None):
        self.table_tensor, self.entries_tensor = _as_bytes_tensor(table), _as_bytes_tensor(entries)
        self.samples_tensor, self.dropped_tensor = _as_bytes_tensor(samples), _as_bytes_tensor(dropped)
        if self.table_tensor.numel() // abi.export_node_dtype.itemsize != self.entries_tensor.numel() // abi.delta_entry_dtype.itemsize:
            raise ValueError("table and entries differ in length")
        self.box_min = tuple(float(v) for v in np.asarray(box_min, dtype=np.float32).reshape(3))
        self.box_max = tuple(float(v) for v in np.asarray(box_max, dtype=np.float32).reshape(3))
        self.max_level = int(max_level)
        self.counts = counts

    @property
    def device(self):
        return self.table_tensor.device

    @property
    def num_nodes(self):
        return self.table_tensor.numel() // abi.export_node_dtype.itemsize

    @property
    def num_samples(self):
        return self.samples_tensor.numel() // abi.point_dtype.itemsize

    @property
    def nodes(self):
        return self.table_tensor.cpu().numpy().view(abi.export_node_dtype)

    @property
    def entries(self):
        return self.entries_tensor.cpu().numpy().view(abi.delta_entry_dtype)

    @property
    def samples(self):
        return self.samples_tensor.cpu().numpy().view(abi.point_dtype)

    @property
    def dropped(self):
        return self.dropped_tensor.cpu().numpy().view(np.uint32)

    def apply(self, held):
        """Rule D9 in numpy: the new cut as an OctreeExport on the host (select "visible") from `held` (the OctreeExport this delta was taken
        against, or None) and this delta — per entry the first numKept samples of its held entry, then its numDelta samples of the delta."""
        tb, en, dl = self.nodes, self.entries, self.samples
        hs = held.samples if held is not None else np.zeros(0, dtype=abi.point_dtype)
        ht = held.nodes if held is not None else np.zeros(0, dtype=abi.export_node_dtype)
        parts = []
        for t in np.nonzero(en["state"] != abi.DELTA_NONE)[0]:
            k, d = int(en["numKept"][t]), int(en["numDelta"][t])
            if k:
                a = int(ht["firstSample"][int(en["held"][t])])
                parts.append(hs[a: a + k])
            if d:
                a = int(en["firstDelta"][t])
                parts.append(dl[a: a + d])
        samples = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)
        return OctreeExport(tb, samples, self.box_min, self.box_max, self.max_level, abi.EXPORT_VISIBLE)

    def pack(self, return_counts=False):
        """This delta with 8-byte samples (rule K5 with the entries): a PackedViewDelta on the host."""
        packed, c = pack_samples(self.nodes, self.samples, self.box_min, self.box_max, self.entries)
        pd = PackedViewDelta(self.nodes, self.entries, packed, self.dropped, self.box_min, self.box_max, self.max_level, self.counts)
        return (pd, c) if return_counts else pd


# ---- packed samples (include/simlod_hip.h, "packed samples"; simlod_amd/csrc/pack_rules.hpp) ------------------------------------------------
PACKED_MAGIC = b"SIMLODP\0"
PACKED_VERSION = 1


def _pack_box(box_min, box_max):
    """(min fp32, size fp32) of rule K7's box; ValueError for what the calls refuse: a corner that is not finite, a box without extent."""
    mn, mx = np.asarray(box_min, np.float32).reshape(3), np.asarray(box_max, np.float32).reshape(3)
    if not (np.isfinite(mn).all() and np.isfinite(mx).all()):
        raise ValueError("the box is not finite")
    with np.errstate(over="ignore"):
        size = (mx - mn).max()
    if not np.isfinite(size) or not size > 0:
        raise ValueError("the box has no extent")
    return mn, np.float32(size)


def _pack_ranges(table, entries, capacity):
    """Rules K5 and K7 per table entry: (the entries that are touched, first, n of each, the error bits)."""
    t = np.asarray(table).view(abi.export_node_dtype).reshape(-1)
    if len(t) == 0:
        raise ValueError("empty table")
    if entries is None:
        on = (t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
        first, n = t["firstSample"].astype(np.uint64), t["numSamples"].astype(np.uint64)
    else:
        e = np.asarray(entries).view(abi.delta_entry_dtype).reshape(-1)
        if len(e) != len(t):
            raise ValueError("table and entries differ in length")
        on = e["state"] != abi.DELTA_NONE
        first, n = e["firstDelta"].astype(np.uint64), e["numDelta"].astype(np.uint64)
    on = on & (n > 0)
    deep = on & (t["level"] > abi.MAX_DEPTH)
    cap = np.uint64(capacity)
    beyond = on & ~deep & ((first > cap) | (n > cap - np.minimum(first, cap)))
    err = (abi.EXPORT_ERR_NODE_COUNT if deep.any() else 0) | (abi.EXPORT_ERR_CAPACITY if beyond.any() else 0)
    idx = np.nonzero(on & ~deep & ~beyond)[0]
    return t, idx, first[idx].astype(np.int64), n[idx].astype(np.int64), err


def _pack_frames(t, idx, mn, size):
    """Rules K1, K2 and K4 per touched entry: leaf, ns, nmin (n x 3, float64), k, the fp32 node size and corner of the voxel decode."""
    level = t["level"][idx].astype(np.int64)
    leaf = (t["flags"][idx] & abi.EXPORT_FLAG_LEAF) != 0
    A = np.stack([t["X"][idx], t["Y"][idx], t["Z"][idx]], axis=1)
    ns = np.ldexp(np.float64(size), -level)
    nmin = mn.astype(np.float64)[None, :] + A.astype(np.float64) * ns[:, None]
    k = np.where(leaf, 8192.0, 128.0) / ns
    fns = (size / np.ldexp(np.float32(1.0), level).astype(np.float32)).astype(np.float32)
    fmin = ((A.astype(np.float32) + np.float32(0.0)) * fns[:, None] + mn[None, :]).astype(np.float32)
    return leaf, ns, nmin, k, fns, fmin


def _pack_expand(first, n):
    """(the sample index, the position in idx of its entry) of every sample of the ranges"""
    ent = np.repeat(np.arange(len(n), dtype=np.int64), n)
    start = np.repeat(np.cumsum(n) - n, n)
    return np.repeat(first, n) + (np.arange(int(n.sum()), dtype=np.int64) - start), ent


def _voxel_axis(fmin, fns, q):
    return (fmin + (fns * (q.astype(np.float32) + np.float32(0.5))) / np.float32(128.0)).astype(np.float32)


def pack_samples(table, samples, box_min, box_max, entries=None, out=None):
    """simlod_pack_samples in numpy (rules K0-K7): -> (the uint64 records, one per element of `samples` — those no range covers keep what `out`
    had, zero without one —, the SimlodPackCounts record).  `entries` (abi.delta_entry_dtype): the ranges of a view delta.  ValueError for what
    the call refuses: an empty table, a box that is not finite or has no extent."""
    mn, size = _pack_box(box_min, box_max)
    smp = np.asarray(samples).view(abi.point_dtype).reshape(-1)
    t, idx, first, n, err = _pack_ranges(table, entries, len(smp))
    packed = np.zeros(len(smp), np.uint64) if out is None else np.asarray(out, np.uint64).copy()
    c = np.zeros((), dtype=abi.pack_counts_dtype)
    c["error"], c["numSamples"] = err, int(n.sum())
    if len(idx):
        leaf, ns, nmin, k, fns, fmin = _pack_frames(t, idx, mn, size)
        si, ent = _pack_expand(first, n)
        p = smp[si]
        lf = leaf[ent]
        lim = np.where(lf, 8192.0, 128.0)
        clamped = np.zeros(len(si), bool)
        inexact = np.zeros(len(si), bool)
        word = (p["color"] & np.uint32(0xFFFFFF)).astype(np.uint64)
        with np.errstate(invalid="ignore", over="ignore"):
            for a, (name, shift) in enumerate((("x", abi.PACK_SHIFT_X), ("y", abi.PACK_SHIFT_Y), ("z", abi.PACK_SHIFT_Z))):
                tt = (p[name].astype(np.float64) - nmin[ent, a]) * k[ent]
                inside = (tt >= 0) & (tt < lim)
                q = np.where(inside, tt, 0.0).astype(np.uint64)
                q = np.where(tt >= lim, (lim - 1).astype(np.uint64), q)
                clamped |= ~inside
                back = _voxel_axis(fmin[ent, a], fns[ent], q)
                inexact |= ~lf & (back.view(np.uint32) != p[name].view(np.uint32))
                word |= q << np.uint64(shift)
        packed[si] = word
        c["numClamped"], c["numInexact"], c["numAlpha"] = int(clamped.sum()), int(inexact.sum()), int(((p["color"] >> 24) != 0xFF).sum())
    return packed, c


def unpack_samples(table, packed, box_min, box_max, entries=None, out=None):
    """simlod_unpack_samples in numpy (rules K3, K4, K8): -> (the samples as abi.point_dtype, one per record of `packed` — those no range
    covers keep what `out` had, zero without one —, the SimlodPackCounts record: numSamples and error)."""
    mn, size = _pack_box(box_min, box_max)
    pk = np.asarray(packed).view(np.uint64).reshape(-1)
    t, idx, first, n, err = _pack_ranges(table, entries, len(pk))
    smp = np.zeros(len(pk), dtype=abi.point_dtype) if out is None else np.asarray(out).view(abi.point_dtype).reshape(-1).copy()
    c = np.zeros((), dtype=abi.pack_counts_dtype)
    c["error"], c["numSamples"] = err, int(n.sum())
    if len(idx):
        leaf, ns, nmin, k, fns, fmin = _pack_frames(t, idx, mn, size)
        si, ent = _pack_expand(first, n)
        w = pk[si]
        lf = leaf[ent]
        mask = np.where(lf, (1 << abi.PACK_POINT_BITS) - 1, (1 << abi.PACK_VOXEL_BITS) - 1).astype(np.uint64)
        step = ns[ent] / 8192.0
        o = np.zeros(len(si), dtype=abi.point_dtype)
        for a, (name, shift) in enumerate((("x", abi.PACK_SHIFT_X), ("y", abi.PACK_SHIFT_Y), ("z", abi.PACK_SHIFT_Z))):
            q = (w >> np.uint64(shift)) & mask
            pt = (nmin[ent, a] + (q.astype(np.float64) + 0.5) * step).astype(np.float32)
            o[name] = np.where(lf, pt, _voxel_axis(fmin[ent, a], fns[ent], q))
        o["color"] = (w & np.uint64(0xFFFFFF)).astype(np.uint32) | np.uint32(0xFF000000)
        smp[si] = o
    return smp, c


class PackedExport:
    """An OctreeExport whose samples are 8-byte records (include/simlod_hip.h, "packed samples"): the table and numSamples x uint64 as uint8
    tensors on the host or on a device, with the box, max_level and select of the export it came from."""

    def __init__(self, table, packed, box_min, box_max, max_level=20, select=abi.EXPORT_ALL):
        self.table_tensor = _as_bytes_tensor(table)
        self.packed_tensor = _as_bytes_tensor(packed)
        if self.table_tensor.numel() % abi.export_node_dtype.itemsize or self.packed_tensor.numel() % 8:
            raise ValueError("table / packed samples are not whole records")
        self.box_min = tuple(float(v) for v in np.asarray(box_min, dtype=np.float32).reshape(3))
        self.box_max = tuple(float(v) for v in np.asarray(box_max, dtype=np.float32).reshape(3))
        self.max_level = int(max_level)
        self.select = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)

    @property
    def num_nodes(self):
        return self.table_tensor.numel() // abi.export_node_dtype.itemsize

    @property
    def num_samples(self):
        return self.packed_tensor.numel() // 8

    @property
    def device(self):
        return self.table_tensor.device

    @property
    def nodes(self):
        return self.table_tensor.cpu().numpy().view(abi.export_node_dtype)

    @property
    def packed(self):
        return self.packed_tensor.cpu().numpy().view(np.uint64)

    def to(self, device):
        return PackedExport(self.table_tensor.to(device), self.packed_tensor.to(device), self.box_min, self.box_max, self.max_level, self.select)

    def unpack(self, return_counts=False):
        """The OctreeExport these records decode to (rule K8, in numpy), on the host.  DeviceOctree.unpack does the same on the device."""
        samples, c = unpack_samples(self.nodes, self.packed, self.box_min, self.box_max)
        ex = OctreeExport(self.nodes, samples, self.box_min, self.box_max, self.max_level, self.select)
        return (ex, c) if return_counts else ex

    def save(self, path):
        h = np.zeros(1, dtype=header_dtype)
        h["magic"], h["version"], h["select"], h["max_level"], h["header_bytes"] = PACKED_MAGIC, PACKED_VERSION, self.select, self.max_level, HEADER_BYTES
        h["numNodes"], h["numSamples"] = self.num_nodes, self.num_samples
        h["box_min"], h["box_max"] = self.box_min, self.box_max
        with open(path, "wb") as f:
            f.write(h.tobytes())
            f.write(self.table_tensor.cpu().numpy().tobytes())
            f.write(self.packed_tensor.cpu().numpy().tobytes())

    @classmethod
    def load(cls, path):
        """Read a file written by save(); header, size and table are checked before the packed export is returned (host tensors)."""
        raw = np.fromfile(path, dtype=np.uint8)
        if raw.size < HEADER_BYTES:
            raise ValueError(f"{path}: truncated header")
        h = raw[:HEADER_BYTES].view(header_dtype)[0]
        if bytes(h["magic"]).ljust(8, b"\0") != PACKED_MAGIC:
            raise ValueError(f"{path}: not a packed octree export (magic)")
        if int(h["version"]) != PACKED_VERSION or int(h["header_bytes"]) != HEADER_BYTES:
            raise ValueError(f"{path}: unsupported version {int(h['version'])}")
        if int(h["select"]) > abi.EXPORT_REGION:
            raise ValueError(f"{path}: unknown selection {int(h['select'])}")
        n, m = int(h["numNodes"]), int(h["numSamples"])
        tb, sb = n * abi.export_node_dtype.itemsize, m * 8
        if raw.size != HEADER_BYTES + tb + sb:
            raise ValueError(f"{path}: {raw.size} bytes, the header announces {HEADER_BYTES + tb + sb}")
        _pack_box(h["box_min"], h["box_max"])
        px = cls(raw[HEADER_BYTES: HEADER_BYTES + tb].copy(), raw[HEADER_BYTES + tb:].copy(), h["box_min"], h["box_max"], int(h["max_level"]), int(h["select"]))
        validate_table(px.nodes, m)
        return px


class PackedViewDelta:
    """A ViewDelta whose samples are 8-byte records: table, entries, numDeltaSamples x uint64 and the dropped list as uint8 tensors."""

    def __init__(self, table, entries, packed, dropped, box_min, box_max, max_level=20, counts=None):
        self.table_tensor, self.entries_tensor = _as_bytes_tensor(table), _as_bytes_tensor(entries)
        self.packed_tensor, self.dropped_tensor = _as_bytes_tensor(packed), _as_bytes_tensor(dropped)
        if self.table_tensor.numel() // abi.export_node_dtype.itemsize != self.entries_tensor.numel() // abi.delta_entry_dtype.itemsize:
            raise ValueError("table and entries differ in length")
        self.box_min = tuple(float(v) for v in np.asarray(box_min, dtype=np.float32).reshape(3))
        self.box_max = tuple(float(v) for v in np.asarray(box_max, dtype=np.float32).reshape(3))
        self.max_level = int(max_level)
        self.counts = counts

    @property
    def device(self):
        return self.table_tensor.device

    @property
    def num_nodes(self):
        return self.table_tensor.numel() // abi.export_node_dtype.itemsize

    @property
    def num_samples(self):
        return self.packed_tensor.numel() // 8

    @property
    def nodes(self):
        return self.table_tensor.cpu().numpy().view(abi.export_node_dtype)

    @property
    def entries(self):
        return self.entries_tensor.cpu().numpy().view(abi.delta_entry_dtype)

    @property
    def packed(self):
        return self.packed_tensor.cpu().numpy().view(np.uint64)

    @property
    def dropped(self):
        return self.dropped_tensor.cpu().numpy().view(np.uint32)

    def to(self, device):
        return PackedViewDelta(*(x.to(device) for x in (self.table_tensor, self.entries_tensor, self.packed_tensor, self.dropped_tensor)),
                               self.box_min, self.box_max, self.max_level, self.counts)

    def unpack(self, return_counts=False):
        """The ViewDelta these records decode to (rule K8, in numpy), on the host."""
        samples, c = unpack_samples(self.nodes, self.packed, self.box_min, self.box_max, self.entries)
        vd = ViewDelta(self.nodes, self.entries, samples, self.dropped, self.box_min, self.box_max, self.max_level, self.counts)
        return (vd, c) if return_counts else vd


class Region:
    """A convex region: up to 16 half-spaces (nx, ny, nz, d) as float32; a point is inside iff nx*x + ny*y + nz*z + d >= 0 for every one.
    No planes: the whole space."""

    def __init__(self, planes=()):
        p = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
        if len(p) > abi.REGION_MAX_PLANES:
            raise ValueError(f"{len(p)} planes: a region has at most {abi.REGION_MAX_PLANES}")
        with np.errstate(over="ignore"):
            self.planes = p.astype(np.float32)
        if not np.isfinite(self.planes).all():
            raise ValueError("a plane coefficient is not finite (as float32)")

    @classmethod
    def from_planes(cls, planes):
        return cls(planes)

    @classmethod
    def from_box(cls, lo, hi):
        """The axis-aligned box lo <= p <= hi: per axis the planes (+e, -lo) and (-e, +hi)."""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        p = np.zeros((6, 4))
        for a in range(3):
            p[2 * a, a], p[2 * a, 3] = 1.0, -lo[a]
            p[2 * a + 1, a], p[2 * a + 1, 3] = -1.0, hi[a]
        return cls(p)

    @classmethod
    def from_frustum(cls, transform):
        """The view frustum's four side planes and w >= 0 of a world-view-projection matrix as the uniforms store it (row-major: clip = M (p, 1)):
        w + x, w - x, w + y, w - y, w."""
        m = np.asarray(transform, dtype=np.float64).reshape(4, 4)
        return cls(np.stack([m[3] + m[0], m[3] - m[0], m[3] + m[1], m[3] - m[1], m[3]]))

    def record(self):
        """The SimlodRegion the C ABI takes (abi.region_dtype, one record)."""
        r = np.zeros(1, dtype=abi.region_dtype)
        r["numPlanes"] = len(self.planes)
        r["planes"][0, : len(self.planes)] = self.planes
        return r


class Clip:
    """What a frame does with a region (include/simlod_hip.h, "clip regions"): mode "inside" shows what is inside it, "outside" cuts it away,
    "highlight" gives what is inside it the colour word `color`; "off" is no clip.  DeviceOctree.set_clip takes one."""

    def __init__(self, region, mode="inside", color=0):
        if not isinstance(region, Region):
            region = Region(region)                                        # (planes: validated there)
        if mode not in abi.CLIP_MODES:
            raise ValueError(f"mode {mode!r}: a clip's mode is one of {sorted(abi.CLIP_MODES)}")
        if not 0 <= int(color) <= 0xFFFFFFFF:
            raise ValueError("a colour word is a 32-bit unsigned integer")
        self.region, self.mode, self.color = region, mode, int(color)

    def record(self):
        """The SimlodClip the C ABI takes (abi.clip_dtype, one record)."""
        r = np.zeros(1, dtype=abi.clip_dtype)
        r["mode"], r["color"] = abi.CLIP_MODES[self.mode], self.color
        r["region"] = self.region.record()
        return r


class Paint:
    """What simlod_paint_region does to the colour word of a sample (include/simlod_hip.h, "paint regions", rules E1-E4): `set` it, `blend` its
    three colour bytes towards a colour, look it up in a 256-entry `ramp` by height, or take it from an `array` in the query's order."""

    def __init__(self, mode, color=0, strength=0, z0=0.0, scale=0.0, table=None):
        self.mode = abi.PAINT_MODES[mode] if isinstance(mode, str) else int(mode)
        if not 0 <= self.mode <= abi.PAINT_ARRAY:
            raise ValueError(f"paint mode {mode!r}")
        if not 0 <= int(color) <= 0xFFFFFFFF:
            raise ValueError("a colour word is a 32-bit unsigned integer")
        self.color, self.strength = int(color), int(strength)
        with np.errstate(over="ignore"):
            self.z0, self.scale = np.float32(z0), np.float32(scale)
        self.table = np.zeros(256, np.uint32) if table is None else np.asarray(table, dtype=np.uint32).reshape(-1).copy()
        if len(self.table) != 256:
            raise ValueError(f"{len(self.table)} table entries: a ramp has 256")
        if self.mode == abi.PAINT_BLEND and not 1 <= self.strength <= 255:
            raise ValueError(f"strength {self.strength}: 1 .. 255")
        if self.mode == abi.PAINT_RAMP and not (np.isfinite(self.z0) and np.isfinite(self.scale) and self.scale > 0):
            raise ValueError("a ramp needs a finite z0 and a finite scale > 0 (as float32)")

    @classmethod
    def set(cls, color):
        """Rule E1: the colour word becomes `color`."""
        return cls(abi.PAINT_SET, color)

    @classmethod
    def blend(cls, color, strength):
        """Rule E2: bytes 0..2 become (c*(256 - strength) + t*strength + 128) >> 8, t that byte of `color`; strength 1 .. 255."""
        return cls(abi.PAINT_BLEND, color, strength)

    @classmethod
    def ramp(cls, z0, z1, table):
        """Rule E3 with scale = float32(256 / (z1 - z0)): the 256 words of `table` spread evenly over z0 <= z < z1, the ends held outside."""
        z0, z1 = float(z0), float(z1)
        if not z1 > z0:
            raise ValueError("a ramp needs z1 > z0")
        return cls(abi.PAINT_RAMP, z0=z0, scale=256.0 / (z1 - z0), table=table)

    @classmethod
    def array(cls):
        """Rule E4: sample j of the query's order gets colors[j] (an undo, or colours computed elsewhere)."""
        return cls(abi.PAINT_ARRAY)

    @classmethod
    def ramp_from(cls, summary, colours, equalize=False):
        """A RAMP paint over the bins `summary` (a Summary) was taken with — its z0 and scale —, so that a sample counted in histZ[i] gets
        table[i].  colours: the palette, lowest height first, any number of words; spread evenly over the 256 bins, or, equalize, by the
        cumulative distribution of the heights (Summary.equalized_table): every colour then covers about the same number of samples."""
        pal = np.asarray(colours, dtype=np.uint32).reshape(-1)
        if len(pal) == 0:
            raise ValueError("a ramp needs a colour")
        table = summary.equalized_table(pal) if equalize else pal[np.arange(256) * len(pal) // 256]
        return cls(abi.PAINT_RAMP, z0=summary.z0, scale=summary.scale, table=table)

    def record(self):
        """The SimlodPaint the C ABI takes (abi.paint_dtype, one record)."""
        r = np.zeros(1, dtype=abi.paint_dtype)
        r["mode"], r["color"], r["strength"], r["z0"], r["scale"] = self.mode, self.color, self.strength, self.z0, self.scale
        r["table"][0] = self.table
        return r

    def ramp_index(self, z):
        """Rule E3's table index of float32 heights, in numpy float64."""
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.asarray(z, np.float32).astype(np.float64) - np.float64(self.z0)) * np.float64(self.scale)
            return np.where(t >= 255.0, 255, np.where(t > 0.0, np.minimum(np.nan_to_num(t, nan=0.0), 255.0), 0.0)).astype(np.int64)

    def apply(self, color, z):
        """The new colour words of samples with the words `color` (uint32) and the heights `z` (float32): rules E1-E3, vectorised."""
        c = np.asarray(color, dtype=np.uint32)
        if self.mode == abi.PAINT_SET:
            return np.full(c.shape, self.color, np.uint32)
        if self.mode == abi.PAINT_BLEND:
            out = c & np.uint32(0xFF000000)
            a = np.uint32(self.strength)
            for sh in (0, 8, 16):
                old, t = (c >> np.uint32(sh)) & np.uint32(0xFF), np.uint32((self.color >> sh) & 0xFF)
                out = out | ((((old * (np.uint32(256) - a) + t * a + np.uint32(128)) >> np.uint32(8))) << np.uint32(sh))
            return out.astype(np.uint32)
        if self.mode == abi.PAINT_RAMP:
            return self.table[self.ramp_index(z)]
        raise ValueError("an ARRAY paint takes its colours from the caller")


class Summary:
    """The SimlodSummary record of one simlod_query_summary call (include/simlod_hip.h, "summary queries"; abi.summary_dtype) — from
    DeviceOctree.summarize_region or its mirror OctreeExport.summarize — with the bins (z0, scale as float32) its z histogram was taken in.
    Every field of the record is exact; what this class derives from it is floating point."""

    def __init__(self, record, z0=0.0, scale=1.0):
        self.record = np.array(record, dtype=abi.summary_dtype).reshape(())
        self.z0, self.scale = np.float32(z0), np.float32(scale)

    def __getitem__(self, name):
        return self.record[name]

    def __eq__(self, other):
        return isinstance(other, Summary) and self.tobytes() == other.tobytes() and (self.z0, self.scale) == (other.z0, other.scale)

    def tobytes(self):
        return self.record.tobytes()

    @property
    def num_samples(self):
        return int(self.record["numSamples"])

    def extent(self):
        """(min, max) per axis as float32[3] (rule S1); with no sample (+inf, -inf)."""
        return self.record["min"].copy(), self.record["max"].copy()

    def centroid(self, box_min, size):
        """The mean position as float64[3], from the sums of the 20-bit cells (rule S2): each sample stands at the middle of its cell of
        size / 2^20 of the box that starts at box_min.  No sample: ValueError."""
        n = self.num_samples
        if n == 0:
            raise ValueError("no sample, no centroid")
        cell = float(size) / abi.SUMMARY_CELLS
        return np.array([float(box_min[k]) + (int(self.record["sum"][k]) / n + 0.5) * cell for k in range(3)], np.float64)

    def covariance(self, size):
        """The 3 x 3 covariance matrix of the positions as float64, from the sums of the products of the 16-bit cells (rule S2).  The
        resolution is that of the 16-bit cell, size / 65536: a sample stands anywhere in its cell, and the mean of the 16-bit cells is taken
        from the 20-bit sum (c16 = c20 >> 4), which is off by less than one 16-bit cell — so an entry is right to about one cell times the
        selection's spread on those axes, and a selection thinner than a cell has no measurable variance on that axis.  No sample: ValueError."""
        n = self.num_samples
        if n == 0:
            raise ValueError("no sample, no covariance")
        cell = float(size) / 65536.0
        mean = [int(self.record["sum"][k]) / (16.0 * n) for k in range(3)]
        m = np.zeros((3, 3), np.float64)
        for j, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            m[a, b] = m[b, a] = (int(self.record["sum2"][j]) / n - mean[a] * mean[b]) * cell * cell
        return m

    def ramp_range(self):
        """(z0, scale) as float32 for the bins of a height ramp over this selection: the lowest z falls into bin 0 and the highest into bin
        255 under rule E3 (scale is the float32 at or above 255 / (max z - min z) whose fp64 product reaches 255).  A selection of one height
        gives (that height, 1).  No sample, or a z extent that is not finite: ValueError."""
        lo, hi = np.float32(self.record["min"][2]), np.float32(self.record["max"][2])
        if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
            raise ValueError("the selection has no finite z extent")
        if hi == lo:
            return lo, np.float32(1.0)
        span = np.float64(hi) - np.float64(lo)
        with np.errstate(over="ignore"):
            scale = np.float32(255.0 / span)
            while np.isfinite(scale) and span * np.float64(scale) < 255.0:
                scale = np.nextafter(scale, np.float32(np.inf))
        if not np.isfinite(scale):
            raise ValueError("the z extent is too small for a float32 scale")
        return lo, scale

    def equalized_table(self, colours):
        """256 colour words from the palette `colours` (lowest height first), bin i taking the colour at the place its samples hold in
        histZ's cumulative distribution — the middle of the bin: index ((2 * samples below + histZ[i]) * len(colours)) // (2 * numSamples), in
        integers.  The index never falls from one bin to the next.  No sample: the palette spread evenly."""
        pal = np.asarray(colours, dtype=np.uint32).reshape(-1)
        if len(pal) == 0:
            raise ValueError("a ramp needs a colour")
        h = [int(v) for v in self.record["histZ"]]
        n = sum(h)
        if n == 0:
            return pal[np.arange(256) * len(pal) // 256]
        idx, below = [], 0
        for v in h:
            idx.append(min(len(pal) - 1, ((2 * below + v) * len(pal)) // (2 * n)))
            below += v
        return pal[np.asarray(idx, np.int64)]


class Compare:
    """The parameters of a compare query (include/simlod_hip.h, "compare queries"; abi.compare_params_dtype): the radius (float32), the 255
    ascending squared-distance thresholds and the 256 colour words of rule C5, the miss colour, and the candidate budget of rule C6
    (max_candidates; None: the device entry points' default — DeviceOctree.compare_samples and compare_region take 64 per sample of A —,
    0: no limit, said explicitly.  record() and the host mirror compare_samples, which launch nothing, read None as the C call's 0)."""

    def __init__(self, radius, thresholds2, table, miss_color=0, max_candidates=None, max_workgroups=0):
        with np.errstate(over="ignore"):
            self.radius = np.float32(radius)
        self.thresholds2 = np.asarray(thresholds2, dtype=np.float64).reshape(-1).copy()
        self.table = np.asarray(table, dtype=np.uint32).reshape(-1).copy()
        self.miss_color, self.max_workgroups = int(miss_color), int(max_workgroups)
        self.max_candidates = None if max_candidates is None else int(max_candidates)
        if not (np.isfinite(self.radius) and self.radius >= 0):
            raise ValueError("a compare query needs a finite radius >= 0 (as float32)")
        if len(self.thresholds2) != 255 or len(self.table) != 256:
            raise ValueError(f"{len(self.thresholds2)} thresholds and {len(self.table)} table entries: 255 and 256")
        if not np.isfinite(self.thresholds2).all() or (np.diff(self.thresholds2) < 0).any():
            raise ValueError("the thresholds are finite and ascending")
        if not 0 <= self.miss_color <= 0xFFFFFFFF or (self.max_candidates is not None and self.max_candidates < 0):
            raise ValueError("a colour word is a 32-bit unsigned integer, a budget is not negative")

    @staticmethod
    def _spread(colours):
        pal = np.asarray(colours, dtype=np.uint32).reshape(-1)
        if len(pal) == 0:
            raise ValueError("a ramp needs a colour")
        return pal[np.arange(256) * len(pal) // 256]

    @classmethod
    def linear(cls, dmax, colours, radius=None, **kw):
        """Bins of equal width in DISTANCE up to dmax: thresholds2[i] = ((i + 1) * dmax / 255)^2 in float64, so a sample at distance dmax or
        beyond gets table[255].  colours: the palette, nearest first, any number of words, spread evenly over the 256 bins.  radius: the search
        radius (None: dmax)."""
        dmax = np.float64(dmax)
        if not (np.isfinite(dmax) and dmax > 0):
            raise ValueError("a linear ramp needs a finite dmax > 0")
        t = (np.arange(1, 256).astype(np.float64) * dmax) / np.float64(255.0)
        return cls(dmax if radius is None else radius, t * t, cls._spread(colours), **kw)

    @classmethod
    def from_summary(cls, summary, colours, radius, **kw):
        """The linear ramp fitted to a previous result: dmax = sqrt(summary maxD2) — the largest distance that result matched (the radius when it
        matched nothing or only coincident samples).  The square root is taken here, on the host; the device takes none."""
        d2 = float(np.asarray(summary)["maxD2"])
        return cls.linear(np.sqrt(d2) if d2 > 0.0 else float(np.float32(radius)) or 1.0, colours, radius=radius, **kw)

    @classmethod
    def from_record(cls, record):
        r = np.asarray(record, dtype=abi.compare_params_dtype).reshape(-1)[0]
        return cls(r["radius"], r["thresholds2"], r["table"], int(r["missColor"]), int(r["maxCandidates"]), int(r["maxWorkgroups"]))

    def __eq__(self, other):
        return isinstance(other, Compare) and self.record().tobytes() == other.record().tobytes()

    def record(self, max_candidates=None):
        """The SimlodCompareParams the C ABI takes (abi.compare_params_dtype, one record); max_candidates overrides the object's."""
        r = np.zeros(1, dtype=abi.compare_params_dtype)
        budget = self.max_candidates if max_candidates is None else int(max_candidates)
        r["radius"], r["missColor"], r["maxCandidates"], r["maxWorkgroups"] = self.radius, self.miss_color, budget or 0, self.max_workgroups
        r["thresholds2"][0], r["table"][0] = self.thresholds2, self.table
        return r

    def index(self, d2):
        """Rule C5's table index of squared distances: the number of thresholds <= d2."""
        return np.searchsorted(self.thresholds2, np.asarray(d2, np.float64), side="right")


def compare_h(radius, size):
    """Rule C4's cell size in float64 from the float32 radius and box size."""
    return max(np.float64(np.float32(radius)) * np.float64(1.0 + 2.0 ** -10), np.float64(np.float32(size)) * np.float64(2.0 ** -20))


def compare_table_slots(num_b):
    """simlod_compare_table_slots: the smallest power of two >= 2 * num_b."""
    s = 2
    while s < 2 * int(num_b):
        s <<= 1
    return s


def compare_home(keys, slots):
    """compare_rules.hpp compare_home: the slot a 60-bit cell key's probing starts at in a table of `slots` (a power of two) slots."""
    log2 = int(slots).bit_length() - 1
    return (np.asarray(keys, np.uint64) * np.uint64(abi.COMPARE_HASH_MUL)) >> np.uint64(64 - log2)


def compare_cells(points, box_min, inv):
    """Rule C4 for an array of abi.point_dtype: (valid, keys) — rule C1's validity and, for the valid samples, the 60-bit key
    cx | cy << 20 | cz << 40 of the cell (0 for the others) — by cell20, the summary mirror's, with rule C4's inv."""
    valid = np.isfinite(points["x"]) & np.isfinite(points["y"]) & np.isfinite(points["z"])
    keys = np.zeros(len(points), np.uint64)
    for k, name in enumerate(("x", "y", "z")):
        keys |= np.where(valid, cell20(points[name], box_min[k], inv), np.uint64(0)) << np.uint64(20 * k)
    return valid, keys


def _compare_pairs(a, b, uniforms_box, radius, max_candidates, count_only, summary_dtype, centres=None, grid_radius=None):
    """What compare_samples and surface_samples share (rules C1, C2, C4, C6, C7): the grid over b's valid samples, the grid's fields of a
    summary record of `summary_dtype` (both summaries keep them, and the budget's error bit, in the same places), and every pair (i, j) of a
    sample of a and a sample of b from its up to 27 cells that passes rule C2 -> (a, b, the record, (pi, pj, [px, py, pz], d2)); the pairs are
    None for a count-only call and when the budget is exceeded.  align_samples passes `centres` — (which samples of a are valid, their
    three float64 coordinate arrays: rule A1's c', held against b in the place of a's own positions) — and `grid_radius` (rule A2: the cell
    size comes from it, the test from `radius`)."""
    a, b = np.asarray(a, dtype=abi.point_dtype).reshape(-1), np.asarray(b, dtype=abi.point_dtype).reshape(-1)
    if not (0 < len(a) <= abi.COMPARE_MAX_COUNT and 0 < len(b) <= abi.COMPARE_MAX_COUNT):
        raise ValueError("numA and numB are 1 .. 2^32 - 2")
    mn, size = _box_of(*uniforms_box)
    if not (np.isfinite(mn).all() and np.isfinite(size) and size > 0):
        raise ValueError("the box needs a finite corner and a finite extent > 0")
    inv = np.float64(1.0) / compare_h(radius if grid_radius is None else grid_radius, size)
    rr = np.float64(radius) * np.float64(radius)
    if centres is None:
        va, ka = compare_cells(a, mn, inv)
        ctr = [a[name].astype(np.float64) for name in ("x", "y", "z")]
    else:
        va, ctr = centres
        ka = np.zeros(len(a), np.uint64)
        for k in range(3):
            ka |= np.where(va, cell20_f64(ctr[k], mn[k], inv), np.uint64(0)) << np.uint64(20 * k)
    vb, kb = compare_cells(b, mn, inv)
    out = np.zeros((), dtype=summary_dtype)
    out["numInvalidA"], out["numInvalidB"] = int((~va).sum()), int((~vb).sum())
    ib = np.flatnonzero(vb)
    ib = ib[np.argsort(kb[ib], kind="stable")]                             # the grid: b's valid samples by cell, ascending index within a cell
    cells, first, pop = np.unique(kb[ib], return_index=True, return_counts=True)
    out["numCells"], out["maxCellPopulation"] = len(cells), int(pop.max()) if len(pop) else 0
    # the up to 27 cells around each valid sample of a: (sample, first grid record, population) per occupied one
    ia = np.flatnonzero(va)
    c = [((ka[ia] >> np.uint64(20 * k)) & np.uint64(0xFFFFF)).astype(np.int64) for k in range(3)]
    who, start, count = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = [c[0] + dx, c[1] + dy, c[2] + dz]
                ok = np.ones(len(ia), bool)
                for v in n:
                    ok &= (v >= 0) & (v < abi.SUMMARY_CELLS)               # (an offset that leaves the grid is skipped, not clamped)
                key = (n[0][ok] | n[1][ok] << 20 | n[2][ok] << 40).astype(np.uint64)
                at = np.searchsorted(cells, key)
                hit = at < len(cells)
                hit[hit] = cells[at[hit]] == key[hit]
                who.append(ia[ok][hit]); start.append(first[at[hit]]); count.append(pop[at[hit]])
    who, start, count = (np.concatenate(v).astype(np.int64) for v in (who, start, count))
    out["numCandidates"] = int(count.sum())
    budget = max_candidates or 0
    if budget != 0 and int(out["numCandidates"]) > budget:
        out["error"] = abi.COMPARE_ERR_BUDGET
    if count_only or int(out["error"]) != 0:
        return a, b, out, None
    # every candidate pair (i, j), then rule C2
    pi = np.repeat(who, count)
    pj = ib[np.repeat(start, count) + (np.arange(len(pi)) - np.repeat(np.cumsum(count) - count, count))]
    d = [b[name][pj].astype(np.float64) - ctr[k][pi] for k, name in enumerate(("x", "y", "z"))]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    ok = d2 <= rr
    return a, b, out, (pi[ok], pj[ok], [v[ok] for v in d], d2[ok])


def compare_samples(a, b, uniforms_box, compare, count_only=False):
    """The host mirror of simlod_compare_samples (include/simlod_hip.h, "compare queries"): a, b arrays of abi.point_dtype, uniforms_box the
    (box_min, box_max) of the uniforms, compare a Compare -> (records as abi.compare_record_dtype, colours as uint32, the summary as one
    abi.compare_summary_dtype record); count_only, or a budget exceeded (rule C6): records and colours are None.  The cells by the same cell20
    the summary's mirror uses, grouped by np.unique over the keys; rules C2, C3 and C5 in numpy float64 and unsigned integers, in the order
    the header gives.  Only the cells rule C4 names are searched, as on the device."""
    a, b, out, pairs = _compare_pairs(a, b, uniforms_box, compare.radius, compare.max_candidates, count_only, abi.compare_summary_dtype)
    if pairs is None:
        return None, None, out
    pi, pj, _, d2 = pairs
    rec = np.zeros(len(a), dtype=abi.compare_record_dtype)
    rec["d2"], rec["nearest"] = np.inf, abi.COMPARE_MISS
    rec["within"] = np.bincount(pi, minlength=len(a))
    order = np.lexsort((pj, d2, pi))                                        # rule C3: per sample the first in (d2, index)
    lead = order[np.r_[True, pi[order][1:] != pi[order][:-1]]] if len(order) else order
    rec["d2"][pi[lead]], rec["nearest"][pi[lead]] = d2[lead], pj[lead]
    matched = rec["within"] != 0
    idx = np.where(matched, compare.index(np.where(matched, rec["d2"], 0.0)), 256)
    colours = np.where(matched, compare.table[np.minimum(idx, 255)], np.uint32(compare.miss_color)).astype(np.uint32)
    out["numMatched"], out["numWithin"] = int(matched.sum()), int(rec["within"].sum(dtype=np.uint64))
    out["maxD2"] = rec["d2"][matched].max() if matched.any() else 0.0
    out["hist"] = np.bincount(idx, minlength=257).astype(np.uint64)
    return rec, colours, out


class CompareResult:
    """What DeviceOctree.compare_region returns: `a`, the selection of A as an OctreeExport (query_region's); `b`, the export of B the
    selection was compared with; `records` (abi.compare_record_dtype, one per sample of a, as bytes) and `colors` (uint32 words) as tensors on
    the device, in a's order; `summary`, one abi.compare_summary_dtype record on the host; the Compare; and the selection's arguments."""

    def __init__(self, a, b, records, colors, summary, compare, selection):
        self.a, self.b, self.records, self.colors, self.summary, self.compare, self.selection = a, b, records, colors, summary, compare, selection

    def records_host(self):
        """The records as a numpy array of abi.compare_record_dtype."""
        return self.records.cpu().numpy().view(abi.compare_record_dtype)

    def nearest_nodes(self):
        """Per sample of a the index, in b's table, of the node that holds its nearest sample (-1: a miss), by a search over firstSample."""
        t = self.b.nodes
        sel = np.flatnonzero(((t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (t["numSamples"] > 0))
        sel = sel[np.argsort(t["firstSample"][sel], kind="stable")]
        near = self.records_host()["nearest"]
        hit = near != abi.COMPARE_MISS
        out = np.full(len(near), -1, np.int64)
        if len(sel):
            out[hit] = sel[np.searchsorted(t["firstSample"][sel], near[hit].astype(np.uint64), side="right") - 1]
        return out

    def paint(self, dev, uniforms, return_previous=False):
        """Write the colours into the octree `dev` the selection was taken from — an ARRAY paint of the same selection, which takes one word
        per sample in the query's order.  Only a result of max_level=20, select="all" has that order.  -> paint_region's result (with
        return_previous the old words too: an ARRAY paint of them is the undo)."""
        s = self.selection
        if s["max_level"] != abi.MAX_DEPTH or s["select"] != "all":
            raise ValueError("only a compare_region(max_level=20, select='all') result is in the order paint_region takes")
        return dev.paint_region(uniforms, s["region"], Paint.array(), footprint=s["footprint"], colors=self.colors, return_previous=return_previous,
                                lasso=s["lasso"], invert=s["invert"])


class Surface:
    """The parameters of a surface query (include/simlod_hip.h, "surface queries"; abi.surface_params_dtype): the radius (float32), the 255
    ascending thresholds and the 256 colour words of rule N8, what the colour is taken from (colour_by: abi.SURFACE_SHADE with the light
    direction, or abi.SURFACE_VARIATION), rule N6's orientation (orient with orient_mode "direction" or "position"), the miss colour of rule
    N9, and the candidate budget of rule C6 (max_candidates; None, 0 and a number as in Compare).  The refusals are the C call's."""

    def __init__(self, radius, thresholds, table, colour_by=abi.SURFACE_SHADE, light=(0.0, 0.0, 1.0), orient=(0.0, 0.0, 1.0), orient_mode="direction",
                 miss_color=0, max_candidates=None, max_workgroups=0):
        with np.errstate(over="ignore"):
            self.radius = np.float32(radius)
            self.light = np.asarray(light, dtype=np.float32).reshape(-1).copy()
            self.orient = np.asarray(orient, dtype=np.float32).reshape(-1).copy()
        self.thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1).copy()
        self.table = np.asarray(table, dtype=np.uint32).reshape(-1).copy()
        self.miss_color, self.max_workgroups, self.colour_by = int(miss_color), int(max_workgroups), int(colour_by)
        self.orient_mode = abi.SURFACE_ORIENT_MODES.get(orient_mode, -1) if isinstance(orient_mode, str) else int(orient_mode)
        self.max_candidates = None if max_candidates is None else int(max_candidates)
        if not (np.isfinite(self.radius) and self.radius >= 0):
            raise ValueError("a surface query needs a finite radius >= 0 (as float32)")
        if len(self.thresholds) != 255 or len(self.table) != 256:
            raise ValueError(f"{len(self.thresholds)} thresholds and {len(self.table)} table entries: 255 and 256")
        if not np.isfinite(self.thresholds).all() or (np.diff(self.thresholds) < 0).any():
            raise ValueError("the thresholds are finite and ascending")
        if self.colour_by not in (abi.SURFACE_SHADE, abi.SURFACE_VARIATION) or self.orient_mode not in (abi.SURFACE_ORIENT_DIRECTION, abi.SURFACE_ORIENT_POSITION):
            raise ValueError("colour_by is SURFACE_SHADE or SURFACE_VARIATION, orient_mode 'direction' or 'position'")
        if len(self.light) != 3 or len(self.orient) != 3 or not (np.isfinite(self.light).all() and np.isfinite(self.orient).all()):
            raise ValueError("light and orient are three finite float32 values")
        if self.colour_by == abi.SURFACE_SHADE and not self.light.any():
            raise ValueError("a hillshade needs a light direction that is not zero")
        if not 0 <= self.miss_color <= 0xFFFFFFFF or (self.max_candidates is not None and self.max_candidates < 0):
            raise ValueError("a colour word is a 32-bit unsigned integer, a budget is not negative")

    @classmethod
    def hillshade(cls, radius, light, colours, orient=(0.0, 0.0, 1.0), orient_mode="direction", **kw):
        """Bins of equal width in the COSINE between the normal and the light: thresholds[i] = c * |c| with c = -1 + (i + 1) / 128, the signed
        squared cosine rule N8 compares.  colours: the palette, facing away first, any number of words, spread evenly over the 256 bins."""
        c = np.float64(-1.0) + np.arange(1, 256).astype(np.float64) / np.float64(128.0)
        return cls(radius, c * np.abs(c), Compare._spread(colours), abi.SURFACE_SHADE, light, orient, orient_mode, **kw)

    @classmethod
    def variation(cls, radius, vmax, colours, **kw):
        """Bins of equal width in the surface variation up to vmax (at most 1/3 is typical): thresholds[i] = (i + 1) * vmax / 255, so a
        neighbourhood at vmax or rougher gets table[255].  colours: the palette, flattest first."""
        vmax = np.float64(vmax)
        if not (np.isfinite(vmax) and vmax > 0):
            raise ValueError("a variation ramp needs a finite vmax > 0")
        return cls(radius, (np.arange(1, 256).astype(np.float64) * vmax) / np.float64(255.0), Compare._spread(colours), abi.SURFACE_VARIATION, **kw)

    @classmethod
    def from_record(cls, record):
        r = np.asarray(record, dtype=abi.surface_params_dtype).reshape(-1)[0]
        if int(r["reserved"]) != 0:
            raise ValueError("the reserved word is 0")
        return cls(r["radius"], r["thresholds"], r["table"], int(r["colourBy"]), r["light"], r["orient"], int(r["orientMode"]), int(r["missColor"]),
                   int(r["maxCandidates"]), int(r["maxWorkgroups"]))

    def __eq__(self, other):
        return isinstance(other, Surface) and self.record().tobytes() == other.record().tobytes()

    def record(self, max_candidates=None):
        """The SimlodSurfaceParams the C ABI takes (abi.surface_params_dtype, one record); max_candidates overrides the object's."""
        r = np.zeros(1, dtype=abi.surface_params_dtype)
        budget = self.max_candidates if max_candidates is None else int(max_candidates)
        r["radius"], r["missColor"], r["maxCandidates"], r["maxWorkgroups"] = self.radius, self.miss_color, budget or 0, self.max_workgroups
        r["colourBy"], r["orientMode"] = self.colour_by, self.orient_mode
        r["thresholds"][0], r["table"][0], r["light"][0], r["orient"][0] = self.thresholds, self.table, self.light, self.orient
        return r

    def index(self, num, den):
        """Rule N8's table index: the number of thresholds with thresholds[i] * den <= num, by the device's binary search (eight steps)."""
        num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
        lo, hi = np.zeros(num.shape, np.int64), np.full(num.shape, 255, np.int64)
        for _ in range(8):                                                 # 255 -> 0 in eight halvings
            mid = (lo + hi) >> 1
            go = (lo < hi) & (self.thresholds[np.minimum(mid, 254)] * den <= num)
            stay = (lo < hi) & ~go
            lo, hi = np.where(go, mid + 1, lo), np.where(stay, mid, hi)
        return lo


def _surface_widen(s):
    """Rule N3's D of an int64 array: the high word times 2^32 (exact) plus the low word, one rounded add."""
    return (s >> np.int64(32)).astype(np.float64) * np.float64(4294967296.0) + (s & np.int64(0xFFFFFFFF)).astype(np.float64)


def _surface_scale(m):
    """Rule N4's P of six arrays (xx, xy, xz, yy, yz, zz) -> (the scaled arrays, m != 0)."""
    big = np.abs(m[0])
    for v in m[1:]:
        big = np.maximum(big, np.abs(v))
    e = (big.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)
    f = ((np.uint64(2046) - e) << np.uint64(52)).view(np.float64)
    return [v * f for v in m], big != 0.0


def _surface_estimates(a, pairs, uniforms_box, surface):
    """Rules N2-N7 for every sample of a at once, in float64 before anything is rounded into a record -> (within, valid, ok, v, lambdaNum,
    lambdaDen, vv): ok marks the samples with an estimate, the others' numbers mean nothing."""
    pi, _, d, _ = pairs
    mn, size = _box_of(*uniforms_box)
    invq = np.float64(abi.SURFACE_Q_SCALE) / compare_h(surface.radius, size)
    n = len(a)
    valid = np.isfinite(a["x"]) & np.isfinite(a["y"]) & np.isfinite(a["z"])
    within = np.bincount(pi, minlength=n).astype(np.int64)
    q = [(v * invq).astype(np.int64) for v in d]                           # rule N2: truncation towards zero
    order = np.argsort(pi, kind="stable")
    first = np.flatnonzero(np.r_[True, pi[order][1:] != pi[order][:-1]]) if len(order) else order
    have = pi[order][first]

    def total(v):                                                           # rule N3: exact integer sums per sample of a
        s = np.zeros(n, np.int64)
        if len(first):
            s[have] = np.add.reduceat(v[order], first)
        return s
    with np.errstate(all="ignore"):
        sx, sy, sz = (_surface_widen(total(v)) for v in q)
        cnt = within.astype(np.float64)
        M = [cnt * _surface_widen(total(q[0] * q[0])) - sx * sx, cnt * _surface_widen(total(q[0] * q[1])) - sx * sy,
             cnt * _surface_widen(total(q[0] * q[2])) - sx * sz, cnt * _surface_widen(total(q[1] * q[1])) - sy * sy,
             cnt * _surface_widen(total(q[1] * q[2])) - sy * sz, cnt * _surface_widen(total(q[2] * q[2])) - sz * sz]
        M, ok = _surface_scale(M)                                           # rule N5
        ok &= valid & (within >= abi.SURFACE_MIN_WITHIN)
        t = (M[0] + M[3]) + M[5]
        B = [t - M[0], -M[1], -M[2], t - M[3], -M[4], t - M[5]]
        for _ in range(abi.SURFACE_SQUARINGS):
            xx, xy, xz, yy, yz, zz = B
            B, nz = _surface_scale([(xx * xx + xy * xy) + xz * xz, (xx * xy + xy * yy) + xz * yz, (xx * xz + xy * yz) + xz * zz,
                                    (xy * xy + yy * yy) + yz * yz, (xy * xz + yy * yz) + yz * zz, (xz * xz + yz * yz) + zz * zz])
            ok &= nz
        xx, xy, xz, yy, yz, zz = B
        j1 = yy > xx                                                        # the first index of the largest diagonal entry
        j2 = zz > np.where(j1, yy, xx)
        v = [np.where(j2, xz, np.where(j1, xy, xx)), np.where(j2, yz, np.where(j1, yy, xy)), np.where(j2, zz, np.where(j1, yz, xz))]
        o = [np.float64(surface.orient[k]) for k in range(3)]               # rule N6
        if surface.orient_mode == abi.SURFACE_ORIENT_POSITION:
            o = [o[k] - a[name].astype(np.float64) for k, name in enumerate(("x", "y", "z"))]
        flip = (v[0] * o[0] + v[1] * o[1]) + v[2] * o[2] < 0.0
        v = [np.where(flip, -c, c) for c in v]
        w = [(M[0] * v[0] + M[1] * v[1]) + M[2] * v[2], (M[1] * v[0] + M[3] * v[1]) + M[4] * v[2], (M[2] * v[0] + M[4] * v[1]) + M[5] * v[2]]   # rule N7
        lnum = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]
        vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        lden = vv * t
    return within, valid, ok, v, lnum, lden, vv


def surface_normals64(a, b, uniforms_box, surface):
    """The mirror's oriented normals BEFORE the record rounds them to float32: (n, 3) float64, zero rows where there is no estimate.  What
    an accuracy check against another eigen-solver compares; the records themselves carry float32."""
    a, b, _, pairs = _compare_pairs(a, b, uniforms_box, surface.radius, 0, False, abi.surface_summary_dtype)
    _, _, ok, v, _, _, _ = _surface_estimates(a, pairs, uniforms_box, surface)
    return np.stack([np.where(ok, c, 0.0) for c in v], -1)


def surface_samples(a, b, uniforms_box, surface, count_only=False):
    """The host mirror of simlod_surface_samples (include/simlod_hip.h, "surface queries"): a, b arrays of abi.point_dtype, uniforms_box the
    (box_min, box_max) of the uniforms, surface a Surface -> (records as abi.surface_record_dtype, colours as uint32, the summary as one
    abi.surface_summary_dtype record); count_only, or a budget exceeded: records and colours are None.  The neighbourhood is compare_samples'
    (the same cells, the same pairs); rules N2 and N3 in int64, rules N4-N8 in numpy float64 over all samples at once, each sum in the order
    the header gives."""
    a, b, out, pairs = _compare_pairs(a, b, uniforms_box, surface.radius, surface.max_candidates, count_only, abi.surface_summary_dtype)
    if pairs is None:
        return None, None, out
    within, valid, ok, v, lnum, lden, vv = _surface_estimates(a, pairs, uniforms_box, surface)
    n = len(a)
    with np.errstate(all="ignore"):
        if surface.colour_by == abi.SURFACE_SHADE:                          # rule N8
            L = [np.float64(surface.light[k]) for k in range(3)]
            al = (v[0] * L[0] + v[1] * L[1]) + v[2] * L[2]
            num, den = al * np.abs(al), vv * ((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
        else:
            num, den = lnum, lden
        idx = np.where(ok, surface.index(np.where(ok, num, 0.0), np.where(ok, den, 0.0)), 256)
        rec = np.zeros(n, dtype=abi.surface_record_dtype)
        for k in range(3):
            rec["normal"][:, k] = np.where(ok, v[k], 0.0).astype(np.float32)
    rec["within"], rec["lambdaNum"], rec["lambdaDen"] = within, np.where(ok, lnum, 0.0), np.where(ok, lden, 0.0)
    colours = np.where(ok, surface.table[np.minimum(idx, 255)], np.uint32(surface.miss_color)).astype(np.uint32)
    out["numEstimated"], out["numDegenerate"] = int(ok.sum()), int((valid & ~ok).sum())
    out["numWithin"] = int(within.sum())
    out["hist"] = np.bincount(idx, minlength=257).astype(np.uint64)
    return rec, colours, out


class SurfaceResult:
    """What DeviceOctree.surface_region returns: `a`, the selection as an OctreeExport (query_region's); `b`, the export it was estimated
    from (a itself unless another octree was given); `records` (abi.surface_record_dtype, one per sample of a, as bytes) and `colors` (uint32
    words) as tensors on the device, in a's order; `summary`, one abi.surface_summary_dtype record on the host; the Surface; and the
    selection's arguments."""

    def __init__(self, a, b, records, colors, summary, surface, selection):
        self.a, self.b, self.records, self.colors, self.summary, self.surface, self.selection = a, b, records, colors, summary, surface, selection

    def records_host(self):
        """The records as a numpy array of abi.surface_record_dtype."""
        return self.records.cpu().numpy().view(abi.surface_record_dtype)

    def unit_normals(self):
        """The normals at length 1 as float64 (n, 3), on the host — the square root and the division the device does not take; a degenerate
        or invalid sample's zero row stays zero."""
        return surface_unit_normals(self.records_host())

    def variation(self):
        """The surface variation lambdaNum / lambdaDen per sample as float64, 0 where the sample is degenerate or invalid."""
        return surface_variation(self.records_host())

    def paint(self, dev, uniforms, return_previous=False):
        """Write the colours into the octree `dev` the selection was taken from — an ARRAY paint of the same selection, as CompareResult.paint.
        Only a result of max_level=20, select="all" has the order that paint takes."""
        s = self.selection
        if s["max_level"] != abi.MAX_DEPTH or s["select"] != "all":
            raise ValueError("only a surface_region(max_level=20, select='all') result is in the order paint_region takes")
        return dev.paint_region(uniforms, s["region"], Paint.array(), footprint=s["footprint"], colors=self.colors, return_previous=return_previous,
                                lasso=s["lasso"], invert=s["invert"])


def surface_unit_normals(records):
    """SurfaceResult.unit_normals for an array of abi.surface_record_dtype."""
    v = np.asarray(records, dtype=abi.surface_record_dtype)["normal"].astype(np.float64).reshape(-1, 3)
    length = np.sqrt((v * v).sum(axis=1))
    return np.divide(v, length[:, None], out=np.zeros_like(v), where=length[:, None] > 0)


def surface_variation(records):
    """SurfaceResult.variation for an array of abi.surface_record_dtype."""
    r = np.asarray(records, dtype=abi.surface_record_dtype).reshape(-1)
    return np.divide(r["lambdaNum"], r["lambdaDen"], out=np.zeros(len(r), np.float64), where=r["lambdaDen"] != 0)


class Cluster:
    """The parameters of a cluster query (include/simlod_hip.h, "cluster queries"; abi.cluster_params_dtype): the radius (float32),
    min_neighbours (rule K3; 1: plain Euclidean clustering), min_cluster_size (rule K7; 1 keeps every cluster), the 256 colour words of rule
    K9 (None: Cluster.palette()), the noise colour, and the candidate budget of rule C6 (max_candidates; None, 0 and a number as in Compare).
    The refusals are the C call's."""

    def __init__(self, radius, min_neighbours=1, min_cluster_size=1, table=None, noise_color=0xFF404040, max_candidates=None, max_workgroups=0):
        with np.errstate(over="ignore"):
            self.radius = np.float32(radius)
        self.min_neighbours, self.min_cluster_size = int(min_neighbours), int(min_cluster_size)
        self.table = (Cluster.palette() if table is None else np.asarray(table, dtype=np.uint32).reshape(-1)).copy()
        self.noise_color, self.max_workgroups = int(noise_color), int(max_workgroups)
        self.max_candidates = None if max_candidates is None else int(max_candidates)
        if not (np.isfinite(self.radius) and self.radius >= 0):
            raise ValueError("a cluster query needs a finite radius >= 0 (as float32)")
        if not (1 <= self.min_neighbours <= 0xFFFFFFFF and 1 <= self.min_cluster_size <= 0xFFFFFFFF):
            raise ValueError("min_neighbours and min_cluster_size are 32-bit unsigned integers >= 1")
        if len(self.table) != 256:
            raise ValueError(f"{len(self.table)} table entries: 256")
        if not 0 <= self.noise_color <= 0xFFFFFFFF or (self.max_candidates is not None and self.max_candidates < 0):
            raise ValueError("a colour word is a 32-bit unsigned integer, a budget is not negative")

    @staticmethod
    def palette():
        """256 distinct opaque colours: the index times an odd constant modulo 2^24 — a bijection, so no two agree — under full alpha."""
        i = np.arange(256, dtype=np.uint64)
        return (((i * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C)) & np.uint64(0xFFFFFF)) | np.uint64(0xFF000000)).astype(np.uint32)

    @classmethod
    def from_record(cls, record):
        r = np.asarray(record, dtype=abi.cluster_params_dtype).reshape(-1)[0]
        if int(r["reserved"]) != 0:
            raise ValueError("the reserved word is 0")
        return cls(r["radius"], int(r["minNeighbours"]), int(r["minClusterSize"]), r["table"], int(r["noiseColor"]), int(r["maxCandidates"]),
                   int(r["maxWorkgroups"]))

    def __eq__(self, other):
        return isinstance(other, Cluster) and self.record().tobytes() == other.record().tobytes()

    def record(self, max_candidates=None):
        """The SimlodClusterParams the C ABI takes (abi.cluster_params_dtype, one record); max_candidates overrides the object's."""
        r = np.zeros(1, dtype=abi.cluster_params_dtype)
        budget = self.max_candidates if max_candidates is None else int(max_candidates)
        r["radius"], r["minNeighbours"], r["minClusterSize"], r["noiseColor"] = self.radius, self.min_neighbours, self.min_cluster_size, self.noise_color
        r["maxCandidates"], r["maxWorkgroups"] = budget or 0, self.max_workgroups
        r["table"][0] = self.table
        return r


def cluster_samples(a, uniforms_box, cluster, count_only=False):
    """The host mirror of simlod_cluster_samples (include/simlod_hip.h, "cluster queries"): a an array of abi.point_dtype, uniforms_box the
    (box_min, box_max) of the uniforms, cluster a Cluster -> (records as abi.cluster_record_dtype, colours as uint32, the summary as one
    abi.cluster_summary_dtype record); count_only, or a budget exceeded: records and colours are None.  The pairs are compare_samples' with
    b = a (rules C1, C2, C4); rule K4's components by passing the minimum label along the core links — of the two labels a link joins the
    higher one's own label becomes the lowest label offered to it — and then replacing every label by its label's label (pointer jumping),
    both until nothing changes: a label only ever decreases and stays inside its component, so it ends at the component's lowest core."""
    a, _, out, pairs = _compare_pairs(a, a, uniforms_box, cluster.radius, cluster.max_candidates, count_only, abi.cluster_summary_dtype)
    if pairs is None:
        return None, None, out
    pi, pj, _, d2 = pairs
    n = len(a)
    valid = np.isfinite(a["x"]) & np.isfinite(a["y"]) & np.isfinite(a["z"])
    within = np.bincount(pi, minlength=n).astype(np.int64)
    core = valid & (within >= cluster.min_neighbours)                       # rule K3
    label = np.arange(n, dtype=np.int64)
    link = core[pi] & core[pj] & (pi > pj)                                  # rule K4 (the pairs hold every link from both its ends: one will do)
    ei, ej = pi[link], pj[link]
    while len(ei):
        li, lj = label[ei], label[ej]                                       # (fully jumped: the labels of labels are themselves)
        open_ = li != lj
        if not open_.any():
            break
        ei, ej, li, lj = ei[open_], ej[open_], li[open_], lj[open_]
        np.minimum.at(label, np.maximum(li, lj), np.minimum(li, lj))        # the higher label's label: the lowest label offered to it
        while True:
            new = label[label]
            if (new == label).all():
                break
            label = new
    root = np.full(n, abi.CLUSTER_MISS, dtype=np.int64)
    root[core] = label[core]
    cand = core[pj] & valid[pi] & ~core[pi]                                 # rule K5: the first core in (d2, index)
    bi, bj, bd = pi[cand], pj[cand], d2[cand]
    order = np.lexsort((bj, bd, bi))
    lead = order[np.r_[True, bi[order][1:] != bi[order][:-1]]] if len(order) else order
    root[bi[lead]] = label[bj[lead]]
    member = root != abi.CLUSTER_MISS
    size_of = np.bincount(root[member], minlength=n).astype(np.int64)       # rule K6, at the root's index
    is_root = core & (label == np.arange(n))
    kept_root = is_root & (size_of >= cluster.min_cluster_size)             # rule K7
    number = np.cumsum(kept_root) - 1                                       # rule K8, at the root's index
    rec = np.zeros(n, dtype=abi.cluster_record_dtype)
    rec["within"] = within
    rec["root"] = root
    safe = np.where(member, root, 0)
    rec["size"] = np.where(member, size_of[safe], 0)
    kept = member & kept_root[safe]
    rec["cluster"] = np.where(kept, number[safe], abi.CLUSTER_NOISE)
    colours = np.where(kept, cluster.table[rec["cluster"] & 255], np.uint32(cluster.noise_color)).astype(np.uint32)   # rule K9
    sizes = size_of[kept_root]
    out["numClusters"], out["numDissolved"] = int(kept_root.sum()), int((is_root & ~kept_root).sum())
    out["numCore"], out["numBorder"], out["numNoise"] = int((kept & core).sum()), int((kept & ~core).sum()), int((~kept).sum())
    out["numWithin"] = int(within.sum())
    if len(sizes):
        out["largestSize"], out["largestCluster"] = int(sizes.max()), int(np.argmax(sizes))      # (argmax: the first, the lowest number)
        out["sizeHist"] = np.bincount(np.floor(np.log2(sizes)).astype(np.int64), minlength=abi.CLUSTER_SIZE_BINS).astype(np.uint64)
    return rec, colours, out


class ClusterResult:
    """What DeviceOctree.cluster_region returns: `a`, the selection as an OctreeExport (query_region's); `records`
    (abi.cluster_record_dtype, one per sample of a, as bytes) and `colors` (uint32 words) as tensors on the device, in a's order; `summary`,
    one abi.cluster_summary_dtype record on the host; the Cluster; and the selection's arguments."""

    def __init__(self, a, records, colors, summary, cluster, selection):
        self.a, self.records, self.colors, self.summary, self.cluster, self.selection = a, records, colors, summary, cluster, selection

    def records_host(self):
        """The records as a numpy array of abi.cluster_record_dtype."""
        r = self.records
        return (r.cpu().numpy() if hasattr(r, "cpu") else np.asarray(r)).view(abi.cluster_record_dtype).reshape(-1)

    @property
    def labels(self):
        """Per sample its cluster's number as int64, -1 for noise and for the members of dissolved clusters."""
        c = self.records_host()["cluster"].astype(np.int64)
        return np.where(c == abi.CLUSTER_NOISE, -1, c)

    def sizes(self):
        """The sizes of the kept clusters, by number (int64, numClusters entries)."""
        rec = self.records_host()
        out = np.zeros(int(self.summary["numClusters"]), np.int64)
        kept = rec["cluster"] != abi.CLUSTER_NOISE
        out[rec["cluster"][kept]] = rec["size"][kept]
        return out

    def members(self, number):
        """The indices in a of the samples of the kept cluster `number`, ascending."""
        return np.flatnonzero(self.records_host()["cluster"] == np.uint32(number))

    def paint(self, dev, uniforms, return_previous=False):
        """Write the colours into the octree `dev` the selection was taken from — an ARRAY paint of the same selection, as CompareResult.paint.
        Only a result of max_level=20, select="all" has that order."""
        s = self.selection
        if s["max_level"] != abi.MAX_DEPTH or s["select"] != "all":
            raise ValueError("only a cluster_region(max_level=20, select='all') result is in the order paint_region takes")
        return dev.paint_region(uniforms, s["region"], Paint.array(), footprint=s["footprint"], colors=self.colors, return_previous=return_previous,
                                lasso=s["lasso"], invert=s["invert"])


IDENTITY_POSE = np.hstack([np.eye(3), np.zeros((3, 1))])


def _pose(pose):
    """A pose as a 3x4 float64 matrix (None: the identity); its entries are finite."""
    T = IDENTITY_POSE.copy() if pose is None else np.array(pose, dtype=np.float64).reshape(3, 4)
    if not np.isfinite(T).all():
        raise ValueError("a pose is a 3x4 matrix of finite entries")
    return T


class Align:
    """The parameters of an align query (include/simlod_hip.h, "align queries"; abi.align_params_dtype) that stay the same over the steps of
    a registration: the radius and the grid's radius (both float32; grid_radius None: the radius — rule A2: one grid serves every radius up
    to grid_radius), the candidate budget of rule C6 (max_candidates as Compare's: None the device entry points' default of 64 per sample
    of A, 0 no limit) and max_workgroups.  The pose and the flags change from call to call and go into record()."""

    def __init__(self, radius, grid_radius=None, max_candidates=None, max_workgroups=0):
        with np.errstate(over="ignore"):
            self.radius = np.float32(radius)
            self.grid_radius = self.radius if grid_radius is None else np.float32(grid_radius)
        self.max_workgroups = int(max_workgroups)
        self.max_candidates = None if max_candidates is None else int(max_candidates)
        if not (np.isfinite(self.radius) and self.radius >= 0):
            raise ValueError("an align query needs a finite radius >= 0 (as float32)")
        if not (np.isfinite(self.grid_radius) and self.grid_radius >= self.radius):
            raise ValueError("the grid's radius is finite and >= the radius (as float32)")
        if self.max_candidates is not None and self.max_candidates < 0:
            raise ValueError("a budget is not negative")

    @classmethod
    def from_record(cls, record):
        r = np.asarray(record, dtype=abi.align_params_dtype).reshape(-1)[0]
        return cls(r["radius"], r["gridRadius"], int(r["maxCandidates"]), int(r["maxWorkgroups"]))

    def __eq__(self, other):
        return isinstance(other, Align) and self.record(None).tobytes() == other.record(None).tobytes()

    def with_radius(self, radius):
        """The same grid with a smaller test radius: what an ICP that tightens its radius passes to its later, reusing steps."""
        return Align(radius, self.grid_radius, self.max_candidates, self.max_workgroups)

    def record(self, pose, flags=0, max_candidates=None):
        """The SimlodAlignParams the C ABI takes (abi.align_params_dtype, one record) for one call: pose a 3x4 matrix (None: the identity),
        flags of abi.ALIGN_COUNT_ONLY and abi.ALIGN_REUSE_GRID; max_candidates overrides the object's."""
        r = np.zeros(1, dtype=abi.align_params_dtype)
        budget = self.max_candidates if max_candidates is None else int(max_candidates)
        r["radius"], r["gridRadius"], r["maxCandidates"], r["maxWorkgroups"] = self.radius, self.grid_radius, budget or 0, self.max_workgroups
        r["pose"][0], r["flags"] = _pose(pose).reshape(-1), int(flags)
        return r


def align_pose_points(points, pose):
    """Rule A1 for an array of abi.point_dtype: (valid, [c'x, c'y, c'z] as float64) — c'_k = ((T_k0*cx + T_k1*cy) + T_k2*cz) + T_k3; valid
    iff x, y and z are finite and all three c'_k are."""
    T = _pose(pose)
    c = [points[name].astype(np.float64) for name in ("x", "y", "z")]
    with np.errstate(invalid="ignore", over="ignore"):
        out = [((T[k, 0] * c[0] + T[k, 1] * c[1]) + T[k, 2] * c[2]) + T[k, 3] for k in range(3)]
    valid = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(out[0]) & np.isfinite(out[1]) & np.isfinite(out[2])
    return valid, out


def align_q(x, box_min, invq):
    """Rule A4 on one axis: (inside, Q as uint64; 0 where outside) of float64 coordinates."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float64) - np.float64(box_min)) * np.float64(invq)
    inside = (t >= 0.0) & (t < abi.ALIGN_Q_SCALE)
    return inside, np.where(inside, t, 0.0).astype(np.uint64)


def align_samples(a, b, uniforms_box, align, pose, count_only=False):
    """The host mirror of simlod_align_samples (include/simlod_hip.h, "align queries"): a, b arrays of abi.point_dtype, uniforms_box the
    (box_min, box_max) of the uniforms, align an Align, pose a 3x4 matrix (None: the identity) -> (records as abi.compare_record_dtype, the
    summary as one abi.align_summary_dtype record); count_only, or a budget exceeded (rule A6): the records are None.  The grid, the
    candidates and the test are _compare_pairs', the compare mirror's, with the posed centres in the place of a's positions; rules A4 and
    A5 in numpy float64 and unsigned 64-bit integers.  A grid is never reused here: a reuse call returns a build call's bytes (rule A9)."""
    a = np.asarray(a, dtype=abi.point_dtype).reshape(-1)
    va, ctr = align_pose_points(a, pose)
    a, b, out, pairs = _compare_pairs(a, b, uniforms_box, align.radius, align.max_candidates, count_only, abi.align_summary_dtype,
                                      centres=(va, ctr), grid_radius=align.grid_radius)
    if pairs is None:
        return None, out
    pi, pj, _, d2 = pairs
    rec = np.zeros(len(a), dtype=abi.compare_record_dtype)
    rec["d2"], rec["nearest"] = np.inf, abi.COMPARE_MISS
    rec["within"] = np.bincount(pi, minlength=len(a))
    order = np.lexsort((pj, d2, pi))                                        # rule C3: per sample the first in (d2, index)
    lead = order[np.r_[True, pi[order][1:] != pi[order][:-1]]] if len(order) else order
    rec["d2"][pi[lead]], rec["nearest"][pi[lead]] = d2[lead], pj[lead]
    matched = rec["within"] != 0
    out["numMatched"], out["numWithin"] = int(matched.sum()), int(rec["within"].sum(dtype=np.uint64))
    out["maxD2"] = rec["d2"][matched].max() if matched.any() else 0.0
    # rules A4, A5 over the matched pairs (c', b[nearest])
    mn, size = _box_of(*uniforms_box)
    invq = np.float64(abi.ALIGN_Q_SCALE) / size
    i, j = np.flatnonzero(matched), rec["nearest"][matched].astype(np.int64)
    inside = np.ones(len(i), bool)
    qa, qb = [], []
    for k, name in enumerate(("x", "y", "z")):
        ia, q = align_q(ctr[k][i], mn[k], invq)
        ib, r = align_q(b[name][j].astype(np.float64), mn[k], invq)
        inside &= ia & ib
        qa.append(q); qb.append(r)
    qa, qb = [q[inside] for q in qa], [q[inside] for q in qb]
    out["numSummed"], out["numOutside"] = int(inside.sum()), int((~inside).sum())
    lo, total = np.uint64(0xFFFFFFFF), lambda v: int(v.sum(dtype=np.uint64))
    for k in range(3):
        out["sumA"][k], out["sumB"][k] = total(qa[k]), total(qb[k])
        for l in range(3):
            P = qa[k] * qb[l]                                               # < 2^48
            out["crossLo"][3 * k + l], out["crossHi"][3 * k + l] = total(P & lo), total(P >> np.uint64(32))
    e = [qb[k].astype(np.int64) - qa[k].astype(np.int64) for k in range(3)]
    E = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).astype(np.uint64)      # < 2^50
    out["sqLo"], out["sqHi"] = total(E & lo), total(E >> np.uint64(32))
    return rec, out


def align_solve(summary, box_min, size):
    """The host's half of an ICP step: the least-squares rigid motion that takes the summed pairs' posed samples of A onto their nearest
    samples of B, from one abi.align_summary_dtype record -> (update: a 3x4 float64 matrix, rms: the pairs' root mean square distance
    before the update, in the box's units), or None with fewer than 3 summed pairs or a second singular value of 0 (the pairs span no
    plane: the rotation is not determined).  N[k][l] = n * cross[k][l] - sumA[k] * sumB[l] is formed in Python integers — exact: n^2 times
    the cross-covariance of the quantised coordinates — and converted to float64 once; numpy.linalg.svd of it, the rotation
    R = V diag(1, 1, det(V U^T)) U^T, the centroids min + (sum / n + 0.5) / invQ (the half step undoes the truncation's bias) and
    t = mu_b - R mu_a."""
    s = np.asarray(summary, dtype=abi.align_summary_dtype).reshape(-1)[0]
    n = int(s["numSummed"])
    if n < 3:
        return None
    sum_a, sum_b = [int(v) for v in s["sumA"]], [int(v) for v in s["sumB"]]
    cross = [(int(h) << 32) + int(l) for l, h in zip(s["crossLo"], s["crossHi"])]
    N = np.array([[float(n * cross[3 * k + l] - sum_a[k] * sum_b[l]) for l in range(3)] for k in range(3)], dtype=np.float64)
    scale = np.abs(N).max()
    if scale == 0.0:
        return None
    U, S, Vt = np.linalg.svd(N / scale)
    if not S[1] > 0.0:
        return None
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0.0 else -1.0])
    R = Vt.T @ D @ U.T
    invq = np.float64(abi.ALIGN_Q_SCALE) / np.float64(np.float32(size))
    mn = np.asarray(box_min, np.float32).astype(np.float64)
    mu_a = mn + (np.array([v / n for v in sum_a]) + 0.5) / invq
    mu_b = mn + (np.array([v / n for v in sum_b]) + 0.5) / invq
    sq = (int(s["sqHi"]) << 32) + int(s["sqLo"])
    return np.hstack([R, (mu_b - R @ mu_a).reshape(3, 1)]), float(np.sqrt(sq / n) / invq)


def compose_pose(update, pose):
    """The pose that applies `pose` first and `update` after it, in float64: [Ru Rp | Ru tp + tu]."""
    u, p = _pose(update), _pose(pose)
    return np.hstack([u[:, :3] @ p[:, :3], (u[:, :3] @ p[:, 3] + u[:, 3]).reshape(3, 1)])


def _pose_corners(pose, corners):
    return corners @ pose[:, :3].T + pose[:, 3]


class AlignResult:
    """What a registration returns: `pose`, the 3x4 float64 matrix that takes A onto B; `summaries`, the abi.align_summary_dtype record of
    every step (host); `rms`, the summed pairs' root mean square distance at every solved step, measured BEFORE that step's update;
    `converged`: the last update moved no corner of A's bounding box by more than the tolerance.  register_region adds `a`, `b` (the
    OctreeExports) and `selection`."""

    def __init__(self, pose, summaries, rms, converged):
        self.pose, self.summaries, self.rms, self.converged = pose, summaries, rms, converged
        self.a = self.b = self.selection = None

    @property
    def steps(self):
        return len(self.summaries)

    def transform(self, samples):
        """The 16-byte samples with their positions moved by the pose — rule A1 in float64, rounded to float32 — and their colours kept: a
        torch tensor of whole records (any dtype, any device) gives a uint8 tensor on its device, anything else a numpy array of
        abi.point_dtype."""
        T = self.pose
        try:
            import torch
        except ImportError:
            torch = None
        if torch is not None and isinstance(samples, torch.Tensor):
            raw = samples.reshape(-1).view(torch.uint8).contiguous().clone()
            f = raw.view(torch.float32).reshape(-1, 4)
            c = [f[:, k].double() for k in range(3)]
            for k in range(3):
                f[:, k] = (((T[k, 0] * c[0] + T[k, 1] * c[1]) + T[k, 2] * c[2]) + T[k, 3]).float()
            return raw
        out = np.array(np.asarray(samples, dtype=abi.point_dtype).reshape(-1), copy=True)
        c = [out[name].astype(np.float64) for name in ("x", "y", "z")]
        with np.errstate(invalid="ignore", over="ignore"):
            for k, name in enumerate(("x", "y", "z")):
                out[name] = (((T[k, 0] * c[0] + T[k, 1] * c[1]) + T[k, 2] * c[2]) + T[k, 3]).astype(np.float32)
        return out


def register_steps(step, box_min, size, corners, pose=None, iterations=30, tol=None):
    """The ICP loop both register_samples (here, on the mirror) and DeviceOctree.register_samples (on the device) run: step(pose, first)
    -> one abi.align_summary_dtype record; align_solve; compose_pose; until the update moves none of `corners` (the 8 corners of A's
    bounding box, under the pose so far) by more than tol (None: size * 2^-22) or `iterations` steps are done.  A step that reports an
    error bit or that align_solve cannot solve ends the loop unconverged.  -> an AlignResult."""
    pose = _pose(pose)
    tol = float(np.float32(size)) * 2.0 ** -22 if tol is None else float(tol)
    corners = np.asarray(corners, np.float64).reshape(-1, 3)
    summaries, rms, converged = [], [], False
    for it in range(int(iterations)):
        s = step(pose, it == 0)
        summaries.append(s)
        solved = None if int(s["error"]) != 0 else align_solve(s, box_min, size)
        if solved is None:
            break
        rms.append(solved[1])
        now = _pose_corners(pose, corners)
        moved = np.abs(_pose_corners(solved[0], now) - now).max() if len(corners) else 0.0
        pose = compose_pose(solved[0], pose)
        if moved <= tol:
            converged = True
            break
    return AlignResult(pose, summaries, rms, converged)


def bounding_corners(points):
    """The 8 corners of the bounding box of the finite samples of an abi.point_dtype array (none finite: no corner)."""
    p = np.asarray(points, dtype=abi.point_dtype).reshape(-1)
    ok = np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])
    if not ok.any():
        return np.zeros((0, 3))
    lo, hi = ([float(f(p[name][ok])) for name in ("x", "y", "z")] for f in (np.min, np.max))
    return np.array([[(lo, hi)[i >> k & 1][k] for k in range(3)] for i in range(8)], dtype=np.float64)


def register_samples(a, b, uniforms_box, align, pose=None, iterations=30, tol=None):
    """The registration of a onto b on the host mirror: register_steps over align_samples.  -> an AlignResult."""
    mn, size = _box_of(*uniforms_box)
    step = lambda T, first: align_samples(a, b, uniforms_box, align, T)[1]
    return register_steps(step, mn, size, bounding_corners(a), pose, iterations, tol)


class Footprint:
    """An extruded polygon (include/simlod_hip.h, "footprint queries"): 3 .. 256 vertices (u, v) as float32, closed from the last to the first,
    in the plane a point is mapped into by u = ((ux*x + uy*y) + uz*z) + u0 and v likewise (axis_u, axis_v as float32).  Inside is the even-odd
    rule F1, so the polygon may be non-convex or cross itself."""

    def __init__(self, vertices, axis_u=(1, 0, 0, 0), axis_v=(0, 1, 0, 0)):
        v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
        if not 3 <= len(v) <= abi.FOOTPRINT_MAX_VERTICES:
            raise ValueError(f"{len(v)} vertices: a footprint has 3 .. {abi.FOOTPRINT_MAX_VERTICES}")
        with np.errstate(over="ignore"):
            self.vertices = v.astype(np.float32)
            self.axis_u = np.asarray(axis_u, dtype=np.float64).reshape(4).astype(np.float32)
            self.axis_v = np.asarray(axis_v, dtype=np.float64).reshape(4).astype(np.float32)
        if not (np.isfinite(self.vertices).all() and np.isfinite(self.axis_u).all() and np.isfinite(self.axis_v).all()):
            raise ValueError("a vertex or an axis coefficient is not finite (as float32)")

    @classmethod
    def from_xy(cls, polygon):
        """A plan-view outline: u = x, v = y, extruded along z."""
        return cls(polygon)

    @classmethod
    def from_rect(cls, lo, hi):
        """The plan-view rectangle from (lo_x, lo_y) to (hi_x, hi_y), clockwise from lo.  By rule F1 as the header states it a point on an
        edge that runs towards smaller v counts as left of it, so this orientation gives lo_x <= x <= hi_x and lo_y <= y < hi_y."""
        lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
        return cls([(lo[0], lo[1]), (lo[0], hi[1]), (hi[0], hi[1]), (hi[0], lo[1])])

    def __len__(self):
        return len(self.vertices)

    def record(self):
        """The SimlodFootprint the C ABI takes (abi.footprint_dtype, one record)."""
        r = np.zeros(1, dtype=abi.footprint_dtype)
        r["numVertices"] = len(self.vertices)
        r["axisU"], r["axisV"] = self.axis_u, self.axis_v
        r["vertices"][0, : len(self.vertices)] = self.vertices
        return r

    def edges(self):
        """(a_u, a_v, b_v, du, dv) per edge as float64 arrays: the edge from a = P[i] to b = P[(i + 1) mod n]."""
        a = self.vertices.astype(np.float64)
        b = np.roll(a, -1, axis=0)
        return a[:, 0], a[:, 1], b[:, 1], b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]

    def project(self, x, y, z):
        """(u, v) of float64 coordinates, in the header's operation order."""
        au, av = self.axis_u.astype(np.float64), self.axis_v.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return ((au[0] * x + au[1] * y) + au[2] * z) + au[3], ((av[0] * x + av[1] * y) + av[2] * z) + av[3]

    def contains_uv(self, u, v):
        """Rule F1 at float64 (u, v): the number of crossed edges is odd."""
        odd = np.zeros(np.shape(u), bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for a_u, a_v, b_v, du, dv in zip(*self.edges()):
                c = du * (v - a_v) - dv * (u - a_u)
                odd ^= ((a_v > v) != (b_v > v)) & ((c > 0) == (dv > 0))
        return odd

    def contains(self, points):
        """Rule F1 on point records (abi.point_dtype) -> a boolean per point."""
        p = np.asarray(points)
        return self.contains_uv(*self.project(*(p[a].astype(np.float64) for a in ("x", "y", "z"))))


def classify_footprint(footprint, nodes, box_min, box_max):
    """Rules F2-F4 of the footprint query for every entry of a table: (near, corner) as boolean arrays — whether the node's projected rectangle
    has a NEAR edge (the node is filtered), and rule F1's verdict at (U_lo, V_lo) (without a NEAR edge: copied if it passes, else outside)."""
    mn, size = _box_of(box_min, box_max)
    s = np.ldexp(size, -nodes["level"].astype(np.int64))[:, None]
    e = np.ldexp(size, -abi.MAX_DEPTH)
    A = np.stack([nodes["X"], nodes["Y"], nodes["Z"]], axis=1).astype(np.float64)
    lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e

    def span(ax):
        ax = ax.astype(np.float64)
        f = [(lo if ax[k] >= 0 else hi)[:, k] for k in range(3)]
        g = [(hi if ax[k] >= 0 else lo)[:, k] for k in range(3)]
        return ((ax[0] * f[0] + ax[1] * f[1]) + ax[2] * f[2]) + ax[3], ((ax[0] * g[0] + ax[1] * g[1]) + ax[2] * g[2]) + ax[3]

    (Ulo, Uhi), (Vlo, Vhi) = span(footprint.axis_u), span(footprint.axis_v)
    near, corner = np.zeros(len(nodes), bool), np.zeros(len(nodes), bool)
    for a_u, a_v, b_v, du, dv in zip(*footprint.edges()):
        pl, ph, ql, qh = du * (Vlo - a_v), du * (Vhi - a_v), dv * (Ulo - a_u), dv * (Uhi - a_u)
        c00, c01, c10, c11 = pl - ql, ph - ql, pl - qh, ph - qh
        far = (max(a_v, b_v) < Vlo) | (min(a_v, b_v) > Vhi) | ((c00 > 0) & (c01 > 0) & (c10 > 0) & (c11 > 0)) | ((c00 < 0) & (c01 < 0) & (c10 < 0) & (c11 < 0))
        near |= ~far
        corner ^= ((a_v > Vlo) != (b_v > Vlo)) & ((c00 > 0) == (dv > 0))
    return near, corner


class Lasso:
    """A polygon on the screen of a perspective camera (include/simlod_hip.h, "lasso queries"): 3 .. 256 vertices (u, v) as float32, closed from
    the last to the first, on the screen a point is mapped onto by the three rows U = ((ux*x + uy*y) + uz*z) + u0, V and W likewise (row_u,
    row_v, row_w as float32): the screen position is (U/W, V/W) where W > 0.  Inside is the even-odd rule L1, multiplied through by W — nothing
    here divides —, so the polygon may be non-convex or cross itself, and a point behind the eye (W <= 0) is never inside."""

    def __init__(self, vertices, row_u, row_v, row_w):
        v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
        if not 3 <= len(v) <= abi.LASSO_MAX_VERTICES:
            raise ValueError(f"{len(v)} vertices: a lasso has 3 .. {abi.LASSO_MAX_VERTICES}")
        with np.errstate(over="ignore"):
            self.vertices = v.astype(np.float32)
            self.row_u, self.row_v, self.row_w = (np.asarray(r, dtype=np.float64).reshape(4).astype(np.float32) for r in (row_u, row_v, row_w))
        if not (np.isfinite(self.vertices).all() and np.isfinite(self.row_u).all() and np.isfinite(self.row_v).all() and np.isfinite(self.row_w).all()):
            raise ValueError("a vertex or a row coefficient is not finite (as float32)")

    @classmethod
    def from_pixels(cls, transform, width, height, pixels):
        """A polygon drawn on the width x height screen of the camera `transform` (row-major world-view-projection M as the uniforms store it):
        vertices in continuous pixel coordinates, pixel (i, j) covering ndc [2i/width - 1, 2(i+1)/width - 1] as Rays.from_pixels states it (its
        centre is (i + 0.5, j + 0.5)).  The rows are width/2 * (M[0] + M[3]), height/2 * (M[1] + M[3]) and M[3], computed in float64 and
        narrowed to float32.  The lasso is what the record says: it agrees with the rasteriser's float32 pixel of a sample to a small fraction
        of a pixel, not bit for bit."""
        m = np.asarray(transform, dtype=np.float64).reshape(4, 4)
        return cls(pixels, 0.5 * float(width) * (m[0] + m[3]), 0.5 * float(height) * (m[1] + m[3]), m[3])

    @classmethod
    def from_ndc(cls, transform, polygon):
        """A polygon in normalised device coordinates (x_clip / w, y_clip / w, each -1 .. 1 on the screen) of the camera `transform`."""
        m = np.asarray(transform, dtype=np.float64).reshape(4, 4)
        return cls(polygon, m[0], m[1], m[3])

    @classmethod
    def from_footprint(cls, footprint):
        """The lasso that selects what `footprint` selects: its axes as rows U and V, and row W = (0, 0, 0, 1)."""
        return cls(footprint.vertices, footprint.axis_u, footprint.axis_v, (0.0, 0.0, 0.0, 1.0))

    def __len__(self):
        return len(self.vertices)

    def record(self):
        """The SimlodLasso the C ABI takes (abi.lasso_dtype, one record)."""
        r = np.zeros(1, dtype=abi.lasso_dtype)
        r["numVertices"] = len(self.vertices)
        r["rowU"], r["rowV"], r["rowW"] = self.row_u, self.row_v, self.row_w
        r["vertices"][0, : len(self.vertices)] = self.vertices
        return r

    def edges(self):
        """(a_u, a_v, b_v, du, dv) per edge as float64 arrays: the edge from a = P[i] to b = P[(i + 1) mod n]."""
        a = self.vertices.astype(np.float64)
        b = np.roll(a, -1, axis=0)
        return a[:, 0], a[:, 1], b[:, 1], b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]

    def edge_block(self):
        """The fp64 block the launcher places in the scratch buffer: {a_u, a_v, du, dv} per edge (n x 4 float64)."""
        a_u, a_v, _, du, dv = self.edges()
        return np.ascontiguousarray(np.stack([a_u, a_v, du, dv], axis=1))

    def project(self, x, y, z):
        """(U, V, W) of float64 coordinates, in the header's operation order."""
        with np.errstate(invalid="ignore", over="ignore"):
            return tuple(((r[0] * x + r[1] * y) + r[2] * z) + r[3] for r in (self.row_u.astype(np.float64), self.row_v.astype(np.float64), self.row_w.astype(np.float64)))

    def contains_uvw(self, U, V, W):
        """Rule L1 at float64 (U, V, W): W > 0 and the number of crossed edges is odd."""
        odd = np.zeros(np.shape(U), bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for a_u, a_v, b_v, du, dv in zip(*self.edges()):
                sa, sb = a_v * W, b_v * W
                c = du * (V - sa) - dv * (U - a_u * W)
                odd ^= ((sa > V) != (sb > V)) & ((c > 0) == (dv > 0))
            return odd & (W > 0)

    def contains(self, points):
        """Rule L1 on point records (abi.point_dtype) -> a boolean per point."""
        p = np.asarray(points)
        return self.contains_uvw(*self.project(*(p[a].astype(np.float64) for a in ("x", "y", "z"))))


def classify_lasso(lasso, nodes, box_min, box_max):
    """Rules L2-L4 of the lasso query for every entry of a table: (outside, copied) as boolean arrays — neither: the node is filtered sample by
    sample (mixed signs of W at its eight corners, or a NEAR edge)."""
    mn, size = _box_of(box_min, box_max)
    s = np.ldexp(size, -nodes["level"].astype(np.int64))[:, None]
    e = np.ldexp(size, -abi.MAX_DEPTH)
    A = np.stack([nodes["X"], nodes["Y"], nodes["Z"]], axis=1).astype(np.float64)
    lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e
    # (U, V, W) at the eight corners: 8 x N
    with np.errstate(invalid="ignore", over="ignore"):
        corners = [lasso.project(*((hi if (k >> a) & 1 else lo)[:, a] for a in range(3))) for k in range(8)]
        U, V, W = (np.stack([c[j] for c in corners]) for j in range(3))
        behind, front = (W <= 0).all(axis=0), (W > 0).all(axis=0)
        near, odd = np.zeros(len(nodes), bool), np.zeros(len(nodes), bool)
        for a_u, a_v, b_v, du, dv in zip(*lasso.edges()):
            sa, sb = a_v * W, b_v * W
            c = du * (V - sa) - dv * (U - a_u * W)
            ua, ub = sa > V, sb > V
            far = (c > 0).all(axis=0) | (c < 0).all(axis=0) | (ua & ub).all(axis=0) | ~(ua | ub).any(axis=0)
            near |= ~far
            odd ^= (ua[0] != ub[0]) & ((c[0] > 0) == (dv > 0))
    outside = behind | (front & ~near & ~odd)
    copied = front & ~near & odd
    return outside, copied


class Profile:
    """A corridor along a polyline (include/simlod_hip.h, "profile queries"): 2 .. 64 vertices (u, v) as float32 and a half-width, in the plane a
    point is mapped into by axis_u / axis_v as a Footprint's; axis_h gives the reported height.  The corridor is the union of one square-ended
    rectangle per segment; where rectangles overlap the lower segment owns the sample."""

    def __init__(self, vertices, half_width, axis_u=(1, 0, 0, 0), axis_v=(0, 1, 0, 0), axis_h=(0, 0, 1, 0)):
        with np.errstate(over="ignore"):
            self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2).astype(np.float32)
            self.half_width = np.float32(half_width)
            self.axis_u, self.axis_v, self.axis_h = (np.asarray(a, dtype=np.float64).reshape(4).astype(np.float32) for a in (axis_u, axis_v, axis_h))
        self._check()

    def _check(self):
        """What rule P6 refuses in a profile, as ValueError."""
        if not 2 <= len(self.vertices) <= abi.PROFILE_MAX_VERTICES:
            raise ValueError(f"{len(self.vertices)} vertices: a profile has 2 .. {abi.PROFILE_MAX_VERTICES}")
        if not (np.isfinite(self.vertices).all() and np.isfinite(self.axis_u).all() and np.isfinite(self.axis_v).all() and np.isfinite(self.axis_h).all()):
            raise ValueError("a vertex or an axis coefficient is not finite (as float32)")
        if not (np.isfinite(self.half_width) and self.half_width > 0):
            raise ValueError("the half-width is not a positive finite float32")
        if (self.vertices[1:] == self.vertices[:-1]).all(axis=1).any():
            raise ValueError("a segment of length zero")

    @classmethod
    def from_xy(cls, polyline, half_width):
        """A plan-view profile: u = x, v = y, h = z."""
        return cls(polyline, half_width)

    def __len__(self):
        return len(self.vertices)

    def reversed(self):
        """The same corridor travelled the other way."""
        return Profile(self.vertices[::-1], self.half_width, self.axis_u, self.axis_v, self.axis_h)

    def record(self):
        """The SimlodProfile the C ABI takes (abi.profile_dtype, one record); ValueError for what the call would refuse (rule P6)."""
        self._check()
        r = np.zeros(1, dtype=abi.profile_dtype)
        r["numVertices"], r["halfWidth"] = len(self.vertices), self.half_width
        r["axisU"], r["axisV"], r["axisH"] = self.axis_u, self.axis_v, self.axis_h
        r["vertices"][0, : len(self.vertices)] = self.vertices
        return r

    def segments(self):
        """The fp64 block of rule P0 (abi.profile_segment_dtype, one row per segment), as the launcher computes it."""
        a = self.vertices.astype(np.float64)
        s = np.zeros(len(a) - 1, dtype=abi.profile_segment_dtype)
        s["au"], s["av"] = a[:-1, 0], a[:-1, 1]
        s["du"], s["dv"] = a[1:, 0] - a[:-1, 0], a[1:, 1] - a[:-1, 1]
        s["L2"] = s["du"] * s["du"] + s["dv"] * s["dv"]
        w = np.float64(self.half_width)
        s["W2"] = (w * w) * s["L2"]
        ln = np.sqrt(s["L2"])
        s["inv"] = 1.0 / ln
        s0 = np.float64(0.0)
        for i in range(len(s)):                               # (s0_(i+1) = s0_i + len_i, one addition at a time)
            s["s0"][i] = s0
            s0 = s0 + ln[i]
        return s

    @property
    def length(self):
        """The polyline's length as rule P0 sums it (float64)."""
        s = self.segments()
        return float(s["s0"][-1] + np.sqrt(s["L2"][-1]))

    def project(self, x, y, z):
        """(u, v) of float64 coordinates, in the header's operation order."""
        au, av = self.axis_u.astype(np.float64), self.axis_v.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return ((au[0] * x + au[1] * y) + au[2] * z) + au[3], ((av[0] * x + av[1] * y) + av[2] * z) + av[3]

    def locate(self, points):
        """Rules P1 and P2 on point records (abi.point_dtype), every point on its own: (segment as int64, -1: in none; station, offset, height as
        float32 — station and offset 0 where the point is in no segment)."""
        p = np.asarray(points)
        x, y, z = (p[a].astype(np.float64) for a in ("x", "y", "z"))
        u, v = self.project(x, y, z)
        ah = self.axis_h.astype(np.float64)
        seg = np.full(len(p), -1, np.int64)
        station, offset = np.zeros(len(p), np.float64), np.zeros(len(p), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            h = ((ah[0] * x + ah[1] * y) + ah[2] * z) + ah[3]
            left = np.arange(len(p))                           # the points in no segment so far
            for i, s in enumerate(self.segments()):
                pu, pv = u[left] - s["au"], v[left] - s["av"]
                al, c = s["du"] * pu + s["dv"] * pv, s["du"] * pv - s["dv"] * pu
                new = (al >= 0) & (al <= s["L2"]) & (c * c <= s["W2"])
                at = left[new]
                seg[at] = i
                station[at] = s["s0"] + al[new] * s["inv"]
                offset[at] = c[new] * s["inv"]
                left = left[~new]
            return seg, station.astype(np.float32), offset.astype(np.float32), h.astype(np.float32)

    def records(self, points):
        """The SimlodProfileSample of every point (abi.profile_sample_dtype): `locate` in the device's layout."""
        seg, station, offset, h = self.locate(points)
        r = np.zeros(len(seg), dtype=abi.profile_sample_dtype)
        r["station"], r["offset"], r["height"] = station, offset, h
        r["segment"] = np.where(seg < 0, abi.PROFILE_NO_SEGMENT, seg).astype(np.uint32)
        return r


def classify_profile(profile, nodes, box_min, box_max):
    """Rule P3 of the profile query for every entry of a table: (far, covered) as boolean arrays — every segment is FAR from the node's projected
    rectangle (the node is outside), some segment COVERS it (the node is copied).  Neither: the node is filtered sample by sample."""
    mn, size = _box_of(box_min, box_max)
    s = np.ldexp(size, -nodes["level"].astype(np.int64))[:, None]
    e = np.ldexp(size, -abi.MAX_DEPTH)
    A = np.stack([nodes["X"], nodes["Y"], nodes["Z"]], axis=1).astype(np.float64)
    lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e

    def span(ax):
        ax = ax.astype(np.float64)
        f = [(lo if ax[k] >= 0 else hi)[:, k] for k in range(3)]
        g = [(hi if ax[k] >= 0 else lo)[:, k] for k in range(3)]
        return ((ax[0] * f[0] + ax[1] * f[1]) + ax[2] * f[2]) + ax[3], ((ax[0] * g[0] + ax[1] * g[1]) + ax[2] * g[2]) + ax[3]

    (Ulo, Uhi), (Vlo, Vhi) = span(profile.axis_u), span(profile.axis_v)
    far, covered = np.ones(len(nodes), bool), np.zeros(len(nodes), bool)
    for sg in profile.segments():
        du, dv, L2, W2 = sg["du"], sg["dv"], sg["L2"], sg["W2"]
        ul, uh, vl, vh = du * (Ulo - sg["au"]), du * (Uhi - sg["au"]), dv * (Vlo - sg["av"]), dv * (Vhi - sg["av"])
        al = np.stack([ul + vl, ul + vh, uh + vl, uh + vh])
        pl, ph, ql, qh = du * (Vlo - sg["av"]), du * (Vhi - sg["av"]), dv * (Ulo - sg["au"]), dv * (Uhi - sg["au"])
        c = np.stack([pl - ql, ph - ql, pl - qh, ph - qh])
        amin, amax, cmin, cmax = al.min(axis=0), al.max(axis=0), c.min(axis=0), c.max(axis=0)
        far &= (amax < 0) | (amin > L2) | ((cmin > 0) & (cmin * cmin > W2)) | ((cmax < 0) & (cmax * cmax > W2))
        covered |= (amin >= 0) & (amax <= L2) & (cmin * cmin <= W2) & (cmax * cmax <= W2)
    return far, covered


def _slab(lo, hi, o, d, tmin, tmax, R):
    """Rule 3 of the ray query for one node's inflated cube [lo, hi] against rays (rows of o, d; tmin, tmax, R per ray) -> a boolean per ray."""
    ok = np.ones(len(o), bool)
    near, far = tmin.copy(), tmax.copy()
    for a in range(3):
        L, H = lo[a] - R, hi[a] + R
        zero = d[:, a] == 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t1, t2 = (L - o[:, a]) / d[:, a], (H - o[:, a]) / d[:, a]
        ok &= ~(zero & ((o[:, a] < L) | (o[:, a] > H)))
        near = np.where(zero, near, np.fmax(near, np.fmin(t1, t2)))
        far = np.where(zero, far, np.fmin(far, np.fmax(t1, t2)))
    return ok & (near <= far)


class Rays:
    """A batch of SimlodRay records (abi.ray_dtype): origin, direction (any non-zero length; t is in units of it), [t_min, t_max], and the cone
    radius + spread * t.  Scalars broadcast over the batch.  Nothing is validated here: an invalid ray is legal input and misses."""

    def __init__(self, origin, direction, t_min=0.0, t_max=1.0, radius=0.0, spread=0.0):
        o = np.asarray(origin, dtype=np.float64).reshape(-1, 3)
        r = np.zeros(len(o), dtype=abi.ray_dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            r["origin"], r["dir"] = o, np.broadcast_to(np.asarray(direction, dtype=np.float64), o.shape)
            r["tMin"], r["tMax"], r["radius"], r["spread"] = t_min, t_max, radius, spread
        self.rays = r

    def __len__(self):
        return len(self.rays)

    @classmethod
    def from_records(cls, records):
        self = cls.__new__(cls)
        self.rays = np.array(np.ascontiguousarray(records).view(abi.ray_dtype).reshape(-1), copy=True)
        return self

    @classmethod
    def vertical(cls, xy, z_top, radius, z_bottom=0.0):
        """Rays straight down from (x, y, z_top) to z_bottom, of constant radius: the height under each position is z_top - hit.t."""
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        o = np.concatenate([xy, np.full((len(xy), 1), float(z_top))], axis=1)
        return cls(o, (0.0, 0.0, -1.0), 0.0, float(z_top) - float(z_bottom), radius, 0.0)

    @classmethod
    def from_pixels(cls, transform, width, height, pixels, pixel_radius=0.5, t_max=None):
        """Cones through pixel centres of the camera `transform` (row-major world-view-projection as the uniforms store it; pixel (i, j) covers
        ndc [2i/width - 1, 2(i+1)/width - 1] as the rasteriser maps it).  The origin is the pixel's point on the near plane, the direction has
        unit length, and radius / spread are pixel_radius times the pixel's footprint there and its growth per unit t.  t_max: None -> the far plane."""
        m = np.linalg.inv(np.asarray(transform, dtype=np.float64).reshape(4, 4))
        px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)

        def unproject(i, j, zc):
            c = np.stack([2.0 * i / width - 1.0, 2.0 * j / height - 1.0, np.full(len(i), zc), np.ones(len(i))], axis=1) @ m.T
            return c[:, :3] / c[:, 3:4]

        i, j = px[:, 0] + 0.5, px[:, 1] + 0.5
        n0, f0, n1, f1 = unproject(i, j, -1.0), unproject(i, j, 1.0), unproject(i + 1.0, j, -1.0), unproject(i + 1.0, j, 1.0)
        length = np.linalg.norm(f0 - n0, axis=1)
        wn, wf = np.linalg.norm(n1 - n0, axis=1), np.linalg.norm(f1 - f0, axis=1)
        return cls(n0, (f0 - n0) / length[:, None], 0.0, length if t_max is None else t_max, pixel_radius * wn, pixel_radius * (wf - wn) / length)

    def record(self):
        """The SimlodRay records the C ABI takes (abi.ray_dtype, one per ray)."""
        return self.rays


def _ray_records(rays):
    return rays.record() if isinstance(rays, Rays) else np.ascontiguousarray(rays).view(abi.ray_dtype).reshape(-1)


def _sphere_records(spheres):
    return spheres.record() if isinstance(spheres, Spheres) else np.ascontiguousarray(spheres).view(abi.sphere_dtype).reshape(-1)


class Spheres:
    """A batch of SimlodSphere records (abi.sphere_dtype): a centre and a radius per query; a scalar radius broadcasts over the batch.  Nothing
    is validated here: an invalid query is legal input and finds nothing."""

    def __init__(self, centers, radius):
        c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        s = np.zeros(len(c), dtype=abi.sphere_dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            s["center"], s["radius"] = c, radius
        self.spheres = s

    def __len__(self):
        return len(self.spheres)

    @classmethod
    def from_records(cls, records):
        self = cls.__new__(cls)
        self.spheres = np.array(np.ascontiguousarray(records).view(abi.sphere_dtype).reshape(-1), copy=True)
        return self

    @classmethod
    def from_points(cls, points, radius):
        """Queries centred on the x, y, z of point records (abi.point_dtype)."""
        p = np.asarray(points)
        return cls(np.stack([p["x"], p["y"], p["z"]], axis=1), radius)

    def record(self):
        """The SimlodSphere records the C ABI takes (abi.sphere_dtype, one per query)."""
        return self.spheres


def validate_table(t, num_samples, buildable=False):
    """Checks of a table against itself (and the sample count): see OctreeExport.validate.  buildable: the device checks of
    simlod_import_octree_buildable too — every entry selected, the leaf flag set exactly on the entries without children, eight children or none."""
    t = np.asarray(t).view(abi.export_node_dtype)
    n = len(t)
    if n == 0:
        raise ValueError("empty table: no root")
    if buildable:
        if ((t["flags"] & abi.EXPORT_FLAG_SELECTED) == 0).any():
            raise ValueError("an entry is not selected: its samples are missing")
        if (((t["flags"] & abi.EXPORT_FLAG_LEAF) != 0) != (t["childMask"] == 0)).any():
            raise ValueError("the leaf flag does not match the children (a truncated export)")
        if ((t["childMask"] != 0) & (t["childMask"] != 0xFF)).any():
            raise ValueError("a node with neither eight children nor none")
    if n > 0xFFFFFFFE:
        raise ValueError("too many nodes")
    level = t["level"].astype(np.int64)
    if (level > abi.MAX_DEPTH).any():
        raise ValueError("level above 20")
    if (t["reserved"] != 0).any() or (t["flags"] & ~np.uint8(abi.EXPORT_FLAG_LEAF | abi.EXPORT_FLAG_SELECTED)).any():
        raise ValueError("reserved bits set")
    r = t[0]
    if int(r["parent"]) != abi.EXPORT_NONE or int(r["level"]) != 0 or int(r["X"]) | int(r["Y"]) | int(r["Z"]):
        raise ValueError("entry 0 is not the root")
    idx = np.arange(n, dtype=np.int64)
    mask = t["childMask"].astype(np.int64)
    kids = _POPCOUNT[mask].astype(np.int64)
    fc = t["firstChild"].astype(np.int64)
    has = mask != 0
    if (fc[~has] != abi.EXPORT_NONE).any():
        raise ValueError("firstChild set without children")
    if has.any():
        if (fc[has] <= idx[has]).any() or (fc[has] + kids[has] > n).any():
            raise ValueError("child index out of range")
        if (level[has] >= abi.MAX_DEPTH).any():
            raise ValueError("children below level 20")
        expect = 1 + np.concatenate([[0], np.cumsum(kids)[:-1]])
        if (fc[has] != expect[has]).any():
            raise ValueError("children not in breadth-first order")
    if 1 + int(kids.sum()) != n:
        raise ValueError("entries that are nobody's child")
    if n > 1:
        c = idx[1:]
        p = t["parent"][1:].astype(np.int64)
        if (p >= c).any():
            raise ValueError("parent index out of range")
        pt = t[p]
        if (level[1:] != pt["level"].astype(np.int64) + 1).any():
            raise ValueError("level does not match the parent's")
        for a in ("X", "Y", "Z"):
            if ((t[a][1:] >> 1) != pt[a]).any():
                raise ValueError(f"coordinate {a} does not match the parent's")
        k = ((t["X"][1:] & 1) << 2 | (t["Y"][1:] & 1) << 1 | (t["Z"][1:] & 1)).astype(np.int64)
        pm = pt["childMask"].astype(np.int64)
        if ((pm >> k) & 1 == 0).any():
            raise ValueError("the parent does not list this octant")
        rank = _POPCOUNT[pm & ((1 << k) - 1)].astype(np.int64)
        if (pt["firstChild"].astype(np.int64) + rank != c).any():
            raise ValueError("the parent lists another entry in this octant")
    ns = t["numSamples"].astype(np.uint64)
    scan = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.uint64)
    if (t["firstSample"] != scan).any():
        raise ValueError("firstSample is not the scan of numSamples")
    if int(ns.sum()) != int(num_samples):
        raise ValueError(f"the table holds {int(ns.sum())} samples, the sample array {int(num_samples)}")
