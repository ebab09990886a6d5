"""Octree export / import on the config-2 stand-in (bench.py's workload: 36 M-point terrain in 1 M batches, exact mode): export ALL, export
CUT@20, import, the buildable import (--buildable: simlod_import_octree_buildable, which also rebuilds the occupancy grids), and a plain
device-to-device copy of the same sample bytes as the ceiling — each timed `--reps` times after a warm-up with device events around the bare C
call.  Prints one JSON line.  Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python ...`.
--region: instead, simlod_query_region CUT@20 on the same octree — the whole box (zero planes) beside simlod_export_octree CUT@20, the two
alternating rep by rep; half the terrain (one oblique plane through the box centre); a city block (a box of 1 % of the area), with its
count-only call — and the device-to-device copy, all in this one run.
--rays: instead, simlod_query_rays CUT@20 on the same octree — one pixel cone through the frame's centre beside the count-only region
query of a thin box around the same ray, the two alternating rep by rep; 4 096 vertical rays of radius 0.5 with their pairs, candidates
and the distinct chunk bytes of the paired nodes — and the device-to-device copy, all in this one run.
--neighbours: instead, simlod_query_neighbours CUT@20 on the same octree — 4 096 queries at random input points, at a radius for which the
host mirror's median `within` (on the first 256 of them) is about 30, with k = 1, 8 and 16 and the count-only call alone — and, for scale, the
--rays case of 4 096 vertical rays and the device-to-device copy, all in this one run.
--footprint: instead, simlod_query_footprint CUT@20 on the same octree — half the terrain (a triangle scaled so that about half the points
pass) with its count-only call; the rectangle of 30-70 % x 20-90 % of the extents beside the same rectangle as a four-plane
simlod_query_region, the two alternating rep by rep; the count-only calls of a 14-vertex and a 256-vertex star, alternating — and the
device-to-device copy, all in this one run.
--lasso: instead, simlod_query_lasso CUT@20 on the same octree — the --footprint polygons (half the terrain, the rectangle, the 14-vertex and
the 256-vertex star) drawn at the terrain's mean height on the bird camera's 1920 x 1080 screen, each alternating rep by rep with
simlod_query_footprint of the plan-view polygon, full and count-only — and the device-to-device copy, all in this one run.  --lasso-only KIND:
that polygon alone (a per-kernel trace of one vertex count).
--inverse: instead, simlod_query_inverse ALL@20 on the same octree — a lasso around the city block of --region (about 1 % of the plan area) and
the half-terrain triangle of --footprint, both on the bird camera's screen — each alternating rep by rep with simlod_export_octree ALL and the
positive simlod_query_lasso ALL@20 of the same polygon, full and count-only, all in this one run.
--profile: instead, simlod_query_profile CUT@20 on the same octree — a 5-vertex polyline across the terrain whose half-width gives the
corridor 1 % of the plan area, with records, without records, and simlod_query_footprint with the corridor's outline polygon, the three
alternating rep by rep; the count-only call — and the device-to-device copy, all in this one run.
--view: instead, simlod_query_view on the same octree under bench.py's bird and close-up cameras at 1920 x 1080 — without a budget beside
simlod_export_octree VISIBLE of the same frame into the same buffers, the two alternating rep by rep; the count-only call; the path the
query replaces, simlod_launch_render + the VISIBLE export — and the device-to-device copy, all in this one run.
--view-delta: instead, simlod_query_view_delta of bench.py's bird camera against four held cuts — the same camera's, the bird camera's orbited by
2 degrees, the close-up camera's, none — each alternating rep by rep with simlod_query_view (full and count-only) of the bird camera; per held
cut the samples sent, the ratios to the two view calls, the count-only delta and the merge — and the device-to-device copy, all in this one run.
--pack: instead, simlod_pack_samples and simlod_unpack_samples of the CUT@20 export and the device-to-device copy of its 16-byte samples, the
three alternating rep by rep (algorithmic bytes: 24 per sample plus the table) — and, for scale on the host it runs on only, the device-to-host
copy of 8 against 16 bytes per sample into page-locked memory.
--paint: instead, simlod_paint_region on the same octree — the whole box, half the terrain and the city block of --region, each as SET without
arrays, BLEND and SET with `previous`; every paint alternates rep by rep with simlod_query_region ALL@20 of the same region (with samples) and
the device-to-device copy (paint, copy, query, copy: both calls start behind the copy); the ratio to the query (expected <= 1.10) and the share
of the copy rate by algorithmic bytes.  --paint-only REGION:MODE: that case alone.
--summary: instead, simlod_query_summary ALL@20 on the same octree — the whole box, half the terrain and the city block of --region; every
summary alternates rep by rep with simlod_query_region ALL@20 of the same region with samples, its count-only call and the device-to-device
copy (each call starts behind the copy); the ratio to the query (the purpose bound: <= 1), the cost over the count-only call and the share of
the copy rate by algorithmic bytes (the selected samples once, plus the table); the whole box again with smaller grids, and once more
after a SET paint of everything (one colour: every lane of a wave on one bin).  --summary-only REGION: that case alone.
--compare: instead, simlod_compare_samples — A the CUT@20 region query of a box of 1/36 of the plan area (about 1 M samples), B the octree's
full CUT@20 export, radius 2.167 as --neighbours' in DESIGN §11: the call with results and the count-only call alternating rep by rep, each
kernel's time from one call between the library's own events, candidates per sample and the largest cell, the rate on the ideal bytes against
the device-to-device copy — and, for scale, the same positions through simlod_query_neighbours at k = 1, in batches of 65 536.  --compare-radius R:
another radius, for cells of hundreds or thousands of samples, without that yardstick.
--compare-whole: the same with A = B = the full export.  --compare-workgroups N: SimlodCompareParams.maxWorkgroups for either.  --surface: with
either, simlod_surface_samples on the same arrays at the same radius as well, alternating with the compare call, and its kernels.  --cluster: with
either, simlod_cluster_samples on A alone at the same radius with minNeighbours 1 and 8, beside simlod_compare_samples(A, A), and its kernels.
--align: with either, simlod_align_samples on the same arrays at the same radius under a small motion: a build call and a reuse call beside the
compare call, their kernels, and a 20-step DeviceOctree.register_samples beside 20 compare calls."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simlod_amd import abi, camera, synthetic  # noqa: E402
from simlod_amd.runtime import DeviceOctree  # noqa: E402

PEAK_GBS = 8000.0


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return float(np.median(ms)), float(ms.min())


def timed_alternating(fns, reps, warmup=2):
    """The median / minimum ms of each of `fns`, run in turns (a, b, a, b, ...) so that a drift of the machine hits all alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for k, fn in enumerate(fns):
            a, b = ev[k][r]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        ms = np.array([a.elapsed_time(b) for a, b in ev[k]])
        out.append((float(np.median(ms)), float(ms.min())))
    return out


def region_bench(dev, u, box, st, reps):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Region, classify_nodes
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = max(int(L.simlod_query_buffer_min_bytes(nn, bound)), int(L.simlod_export_buffer_min_bytes(nn, bound)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    n = np.array([0.6, 0.8, 0.1])
    regions = {"whole_box": Region(), "half_terrain": Region.from_planes([[*n, -float(n @ (b / 2))]]),
               "city_block": Region.from_box((0.45 * b[0], 0.45 * b[1], -1.0), (0.55 * b[0], 0.55 * b[1], b[2] + 1.0))}
    records = {k: r.record() for k, r in regions.items()}

    def query(kind, count_only=False):
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records[kind].ctypes.data), 20, abi.EXPORT_CUT, p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def export_cut():
        rc = L.simlod_export_octree(p(dev.nodes), p(dev.stats), 20, abi.EXPORT_CUT, p(scratch), ctypes.c_uint64(need), p(table), nn, p(samples),
                                    ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    # the two calls alternate, so each runs behind the other's sample copy; the plain copy is timed on its own, as in the export bench (behind
    # a 1.1 GB copy through the caches the single-workgroup walk of whichever call comes next finds its nodes in HBM: 40 us more)
    t_query, t_cut = timed_alternating([lambda: query("whole_box"), export_cut], reps)
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)},
           "export_cut20": {"ms": round(t_cut[0], 4), "ms_min": round(t_cut[1], 4)}}

    def row(kind, ms):
        query(kind)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        assert int(c["error"]) == 0
        t = table[: int(c["numNodes"]) * 40].cpu().numpy().view(abi.export_node_dtype)
        # the share of the candidates that lie in filtered nodes: the result's table holds the counts AFTER the test, so ask a zero-plane
        # query for the counts before it and classify its entries on the host
        outside, inside = classify_nodes(regions[kind].planes, t, u["boxMin"], u["boxMax"])
        query("whole_box", count_only=True)
        torch.cuda.synchronize()
        full = table.cpu().numpy().view(abi.export_node_dtype)
        key = lambda a: (a["level"].astype(np.uint64) << np.uint64(60)) | (a["X"].astype(np.uint64) << np.uint64(40)) | (a["Y"].astype(np.uint64) << np.uint64(20)) | a["Z"].astype(np.uint64)
        before = dict(zip(key(full).tolist(), full["numSamples"].tolist()))
        sel = (t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
        cand = np.array([before[k] for k in key(t).tolist()], dtype=np.int64) * (sel & ~outside)
        assert int(cand.sum()) == int(c["numCandidates"])
        f = float(cand[~inside].sum()) / max(int(c["numCandidates"]), 1)
        nbytes = int(c["numCandidates"]) * 16 + int(c["numSamples"]) * 16 + int(c["numNodes"]) * 40
        gbs = nbytes / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "nodes_listed": int(c["numNodes"]), "nodes_copied": int(c["numCopiedNodes"]),
                "nodes_filtered": int(c["numFilteredNodes"]), "numCandidates": int(c["numCandidates"]), "numSamples": int(c["numSamples"]),
                "f_candidates_in_filtered_nodes": round(f, 4), "algorithmic_bytes": nbytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4)}

    out["whole_box"] = row("whole_box", t_query)
    out["whole_box"]["over_export_cut20"] = round(t_query[0] / t_cut[0], 4)
    out["whole_box"]["bound"] = "t_query <= 1.10 * t_cut of the same run"
    out["whole_box"]["bound_held"] = bool(t_query[0] <= 1.10 * t_cut[0])
    t_half, t_half_count = timed_alternating([lambda: query("half_terrain"), lambda: query("half_terrain", True)], reps)
    out["half_terrain"] = row("half_terrain", t_half)
    out["half_terrain"]["count_only_ms"] = round(t_half_count[0], 4)
    out["half_terrain"]["target"] = ">= 50 % of the copy rate"
    out["half_terrain"]["target_held"] = bool(out["half_terrain"]["frac_of_copy"] >= 0.5)
    t_block, t_block_count = timed_alternating([lambda: query("city_block"), lambda: query("city_block", True)], reps)
    out["city_block"] = row("city_block", t_block)
    out["city_block"]["count_only_ms"] = round(t_block_count[0], 4)
    print(json.dumps(out))


def paint_bench(dev, u, box, st, reps, only=None):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Paint, Region, classify_nodes
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = int(L.simlod_paint_buffer_min_bytes(nn, bound))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    previous = torch.empty(bound, dtype=torch.int32, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    n = np.array([0.6, 0.8, 0.1])
    regions = {"whole_box": Region(), "half_terrain": Region.from_planes([[*n, -float(n @ (b / 2))]]),
               "city_block": Region.from_box((0.45 * b[0], 0.45 * b[1], -1.0), (0.55 * b[0], 0.55 * b[1], b[2] + 1.0))}
    records = {k: r.record() for k, r in regions.items()}
    paints = {"set": (Paint.set(0xFF2060E0).record(), False), "blend": (Paint.blend(0x002060E0, 64).record(), False),
              "set_previous": (Paint.set(0xFF2060E0).record(), True)}

    def paint(kind, mode):
        rec, prev = paints[mode]
        rc = L.simlod_paint_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records[kind].ctypes.data), None, ctypes.c_void_p(rec.ctypes.data), p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None, p(previous) if prev else None, ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def query(kind, count_only=False):
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records[kind].ctypes.data), 20, abi.EXPORT_ALL, p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    out = {"points": int(st["numPoints"]), "numNodes": nn, "numSamples": bound, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "lib": os.environ.get("SIMLOD_HIP_LIB", "product"), "bound": "t_paint <= 1.10 * t_query of the same run"}
    for kind in regions:
        # the candidates in filtered nodes: the classes on the host from a zero-plane count-only call's table (the counts before the test)
        query("whole_box", count_only=True)
        torch.cuda.synchronize()
        full = table.cpu().numpy().view(abi.export_node_dtype)
        outside, inside = classify_nodes(regions[kind].planes, full, u["boxMin"], u["boxMax"])
        cand_filtered = int(full["numSamples"][~outside & ~inside].astype(np.int64).sum())
        out[kind] = {}
        for mode in paints:
            if only is not None and only != f"{kind}:{mode}":
                continue
            # paint, copy, query, copy: both calls run behind the 1.1 GB copy, which leaves neither the nodes nor the region's chunks in the
            # caches (behind the paint of the same region the query would find them there)
            copy = lambda: copy_dst.copy_(copy_src)
            t_paint, t_copy, t_query, _ = timed_alternating([lambda: paint(kind, mode), copy, lambda: query(kind), copy], reps)
            paint(kind, mode)
            torch.cuda.synchronize()
            c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
            assert int(c["error"]) == 0
            painted, cand = int(c["numSamples"]), int(c["numCandidates"])
            copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
            # what the call has to move: the filtered candidates are read for the count, every sample that is read for its colour 16 bytes
            # (SET without previous reads no copied chunk), 4 bytes written per painted sample and 4 more for `previous`, the table
            read = cand_filtered if mode == "set" else cand
            nbytes = read * 16 + painted * (8 if mode == "set_previous" else 4) + int(c["numNodes"]) * 40
            qbytes = cand * 16 + painted * 16 + int(c["numNodes"]) * 40
            gbs = nbytes / (t_paint[0] * 1e6)
            out[kind][mode] = {"ms": round(t_paint[0], 4), "ms_min": round(t_paint[1], 4), "query_all20_ms": round(t_query[0], 4), "d2d_copy_ms": round(t_copy[0], 4),
                               "d2d_copy_GBs": round(copy_gbs, 1), "over_query": round(t_paint[0] / t_query[0], 4), "bound_held": bool(t_paint[0] <= 1.10 * t_query[0]),
                               "numSamples": painted, "numCandidates": cand, "candidates_in_filtered_nodes": cand_filtered, "nodes_copied": int(c["numCopiedNodes"]),
                               "nodes_filtered": int(c["numFilteredNodes"]), "algorithmic_bytes": nbytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4),
                               "query_algorithmic_bytes": qbytes, "query_frac_of_copy": round(qbytes / (t_query[0] * 1e6) / copy_gbs, 4)}
    print(json.dumps(out))


def summary_bench(dev, u, box, st, reps, only=None):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Paint, Region
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = max(int(L.simlod_summary_buffer_min_bytes(nn, bound)), int(L.simlod_paint_buffer_min_bytes(nn, bound)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    record = torch.zeros(abi.summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    n = np.array([0.6, 0.8, 0.1])
    regions = {"whole_box": Region(), "half_terrain": Region.from_planes([[*n, -float(n @ (b / 2))]]),
               "city_block": Region.from_box((0.45 * b[0], 0.45 * b[1], -1.0), (0.55 * b[0], 0.55 * b[1], b[2] + 1.0))}
    records = {k: r.record() for k, r in regions.items()}
    params = {}
    for wg in (0, 256, 512):
        params[wg] = np.zeros(1, dtype=abi.summary_params_dtype)
        params[wg]["z0"], params[wg]["scale"], params[wg]["maxWorkgroups"] = 0.0, 256.0 / b[2], wg

    def summary(kind, wg=0):
        rc = L.simlod_query_summary(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records[kind].ctypes.data), None, ctypes.c_void_p(params[wg].ctypes.data), 20,
                                    abi.EXPORT_ALL, p(scratch), ctypes.c_uint64(need), p(table), nn, p(record), p(counts), stream)
        assert rc == 0

    def query(kind, count_only=False):
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records[kind].ctypes.data), 20, abi.EXPORT_ALL, p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    copy = lambda: copy_dst.copy_(copy_src)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "numSamples": bound, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "lib": os.environ.get("SIMLOD_HIP_LIB", "product"), "bound": "t_summary <= t_query (with samples) of the same run", "target": ">= 50 % of the copy rate"}

    def row(kind):
        # summary, copy, query, copy, count-only, copy: every call runs behind the 1.1 GB copy, which leaves neither the nodes nor the region's
        # chunks in the caches
        t_sum, t_copy, t_query, _, t_count, _ = timed_alternating([lambda: summary(kind), copy, lambda: query(kind), copy, lambda: query(kind, True), copy], reps)
        summary(kind)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        r = record.cpu().numpy().view(abi.summary_dtype)[0]
        assert int(c["error"]) == 0 and int(r["numSamples"]) == int(c["numSamples"]) == int(r["histZ"].sum())
        copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
        nbytes = int(c["numSamples"]) * 16 + int(c["numNodes"]) * 40
        gbs = nbytes / (t_sum[0] * 1e6)
        return {"ms": round(t_sum[0], 4), "ms_min": round(t_sum[1], 4), "query_all20_ms": round(t_query[0], 4), "count_only_ms": round(t_count[0], 4),
                "new_kernels_ms": round(t_sum[0] - t_count[0], 4), "d2d_copy_ms": round(t_copy[0], 4), "d2d_copy_GBs": round(copy_gbs, 1),
                "over_query": round(t_sum[0] / t_query[0], 4), "bound_held": bool(t_sum[0] <= t_query[0]), "numSamples": int(c["numSamples"]),
                "numCandidates": int(c["numCandidates"]), "nodes_copied": int(c["numCopiedNodes"]), "nodes_filtered": int(c["numFilteredNodes"]),
                "algorithmic_bytes": nbytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4), "target_held": bool(gbs / copy_gbs >= 0.5),
                "bins_used": {"histZ": int((r["histZ"] > 0).sum()), "histC": [int((h > 0).sum()) for h in r["histC"]]}}

    for kind in regions:
        if only is None or only == kind:
            out[kind] = row(kind)
    if only is None:
        grids = [256, 512, 0]
        t = timed_alternating([f for wg in grids for f in ((lambda wg=wg: summary("whole_box", wg)), copy)], reps)
        out["whole_box_by_grid_ms"] = {str(wg) if wg else "library": round(t[2 * k][0], 4) for k, wg in enumerate(grids)}
    if only is None or only == "whole_box_one_colour":
        rec = Paint.set(0xFF2060E0).record()
        rc = L.simlod_paint_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(records["whole_box"].ctypes.data), None, ctypes.c_void_p(rec.ctypes.data), p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None, None, ctypes.c_uint64(0), p(counts), stream)
        assert rc == 0
        params[0]["z0"], params[0]["scale"] = -1000.0, 1000.0            # every height in bin 255
        out["whole_box_one_colour"] = row("whole_box")
    print(json.dumps(out))


def footprint_bench(dev, u, box, st, reps):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Footprint, Region, classify_footprint
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = int(L.simlod_footprint_buffer_min_bytes(nn, bound))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)

    def star(n):
        k = np.arange(2 * n)
        r = np.where(k % 2 == 0, 0.45, 0.15) * min(b[0], b[1])
        return Footprint.from_xy(np.stack([b[0] / 2 + r * np.cos(k * np.pi / n), b[1] / 2 + r * np.sin(k * np.pi / n)], axis=1))

    tri = 0.5 + (np.array([(50 / 600, 50 / 400), (550 / 600, 80 / 400), (250 / 600, 380 / 400)]) - 0.5) * 1.25
    rect_lo, rect_hi = (0.3 * b[0], 0.2 * b[1]), (0.7 * b[0], 0.9 * b[1])
    prints = {"half_terrain": Footprint.from_xy(tri * b[:2]), "rect": Footprint.from_rect(rect_lo, rect_hi), "star7": star(7), "star128": star(128)}
    records = {k: f.record() for k, f in prints.items()}
    none = Region().record()
    planes = Region.from_box((*rect_lo, -1.0), (*rect_hi, b[2] + 1.0)).record()
    planes["numPlanes"] = 4                                                      # the x and y planes: the rectangle alone

    def query(kind, count_only=False):
        rc = L.simlod_query_footprint(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), ctypes.c_void_p(records[kind].ctypes.data), 20,
                                      abi.EXPORT_CUT, p(scratch), ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples),
                                      ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def region_rect():
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(planes.ctypes.data), 20, abi.EXPORT_CUT, p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def read_counts():
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0].copy()
        assert int(c["error"]) == 0
        return c

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)}}

    def row(kind, ms, c):
        nbytes = int(c["numCandidates"]) * 16 + int(c["numSamples"]) * 16 + int(c["numNodes"]) * 40
        gbs = nbytes / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "vertices": len(prints[kind]) if kind in prints else 0, "nodes_listed": int(c["numNodes"]),
                "nodes_copied": int(c["numCopiedNodes"]), "nodes_filtered": int(c["numFilteredNodes"]), "numCandidates": int(c["numCandidates"]),
                "numSamples": int(c["numSamples"]), "algorithmic_bytes": nbytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4)}

    def f_of(kind):
        # the share of the candidates that lie in filtered nodes (the table holds the counts after the test: ask a covering query for those before it)
        query(kind)
        c = read_counts()
        t = table[: int(c["numNodes"]) * 40].cpu().numpy().view(abi.export_node_dtype)
        near, corner = classify_footprint(prints[kind], t, u["boxMin"], u["boxMax"])
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), 20, abi.EXPORT_CUT, p(scratch),
                                   ctypes.c_uint64(need), p(table), nn, None, ctypes.c_uint64(0), p(counts), stream)
        assert rc == 0
        torch.cuda.synchronize()
        full = table.cpu().numpy().view(abi.export_node_dtype)
        key = lambda a: (a["level"].astype(np.uint64) << np.uint64(60)) | (a["X"].astype(np.uint64) << np.uint64(40)) | (a["Y"].astype(np.uint64) << np.uint64(20)) | a["Z"].astype(np.uint64)
        before = dict(zip(key(full).tolist(), full["numSamples"].tolist()))
        sel = (t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
        cand = np.array([before[k] for k in key(t).tolist()], dtype=np.int64) * (sel & (near | corner))
        assert int(cand.sum()) == int(c["numCandidates"])
        return round(float(cand[near].sum()) / max(int(c["numCandidates"]), 1), 4), c

    t_half, t_half_count = timed_alternating([lambda: query("half_terrain"), lambda: query("half_terrain", True)], reps)
    f, c = f_of("half_terrain")
    out["half_terrain"] = row("half_terrain", t_half, c)
    out["half_terrain"].update({"count_only_ms": round(t_half_count[0], 4), "f_candidates_in_filtered_nodes": f, "target": ">= 50 % of the copy rate",
                                "target_held": bool(out["half_terrain"]["frac_of_copy"] >= 0.5)})
    t_rect, t_planes = timed_alternating([lambda: query("rect"), region_rect], reps)
    f, c = f_of("rect")
    out["rect"] = row("rect", t_rect, c)
    out["rect"]["f_candidates_in_filtered_nodes"] = f
    region_rect()
    out["rect_as_four_planes"] = row("planes", t_planes, read_counts())
    out["rect"]["over_four_planes"] = round(t_rect[0] / t_planes[0], 4)
    t7, t128 = timed_alternating([lambda: query("star7", True), lambda: query("star128", True)], reps)
    for kind, t in (("star7", t7), ("star128", t128)):
        query(kind, True)
        out[kind + "_count_only"] = row(kind, t, read_counts())
    print(json.dumps(out))


def lasso_bench(dev, u, box, st, reps, T, width, height, only=None):
    """The --footprint cases as lassos on the screen of the camera T: each plan-view polygon is drawn at the terrain's mean height and projected
    to pixels, so the lasso selects about what the footprint selects; lasso and footprint of a case alternate rep by rep, full and count-only."""
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Footprint, Lasso, Region
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = int(L.simlod_lasso_buffer_min_bytes(nn, bound))
    assert need == int(L.simlod_footprint_buffer_min_bytes(nn, bound))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    m = np.asarray(T, dtype=np.float64).reshape(4, 4)

    def star(n):
        k = np.arange(2 * n)
        r = np.where(k % 2 == 0, 0.45, 0.15) * min(b[0], b[1])
        return np.stack([b[0] / 2 + r * np.cos(k * np.pi / n), b[1] / 2 + r * np.sin(k * np.pi / n)], axis=1)

    def on_screen(xy):
        h = np.concatenate([xy, np.full((len(xy), 1), 0.5 * b[2]), np.ones((len(xy), 1))], axis=1) @ m.T
        assert (h[:, 3] > 0).all()
        return np.stack([0.5 * width * (h[:, 0] / h[:, 3] + 1.0), 0.5 * height * (h[:, 1] / h[:, 3] + 1.0)], axis=1)

    tri = 0.5 + (np.array([(50 / 600, 50 / 400), (550 / 600, 80 / 400), (250 / 600, 380 / 400)]) - 0.5) * 1.25
    rect_lo, rect_hi = (0.3 * b[0], 0.2 * b[1]), (0.7 * b[0], 0.9 * b[1])
    plan = {"half_terrain": tri * b[:2], "rect": Footprint.from_rect(rect_lo, rect_hi).vertices.astype(np.float64), "star7": star(7), "star128": star(128)}
    if only is not None:
        plan = {only: plan[only]}
    prints = {k: Footprint.from_xy(v) for k, v in plan.items()}
    lassos = {k: Lasso.from_pixels(T, width, height, on_screen(v)) for k, v in plan.items()}
    frec, lrec = {k: f.record() for k, f in prints.items()}, {k: l.record() for k, l in lassos.items()}
    none = Region().record()

    def query(call, rec, count_only=False):
        rc = call(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), ctypes.c_void_p(rec.ctypes.data), 20, abi.EXPORT_CUT, p(scratch),
                  ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def read_counts():
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0].copy()
        assert int(c["error"]) == 0
        return c

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "screen": [width, height],
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)}}

    def row(kind, ms, ms_count, c):
        nbytes = int(c["numCandidates"]) * 16 + int(c["numSamples"]) * 16 + int(c["numNodes"]) * 40
        gbs = nbytes / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "count_only_ms": round(ms_count[0], 4), "vertices": len(prints[kind]),
                "nodes_listed": int(c["numNodes"]), "nodes_copied": int(c["numCopiedNodes"]), "nodes_filtered": int(c["numFilteredNodes"]),
                "numCandidates": int(c["numCandidates"]), "numSamples": int(c["numSamples"]), "algorithmic_bytes": nbytes, "GBs": round(gbs, 1),
                "frac_of_copy": round(gbs / copy_gbs, 4)}

    for kind in plan:
        ql, qf = L.simlod_query_lasso, L.simlod_query_footprint
        t_l, t_f, t_lc, t_fc = timed_alternating([lambda: query(ql, lrec[kind]), lambda: query(qf, frec[kind]), lambda: query(ql, lrec[kind], True),
                                                  lambda: query(qf, frec[kind], True)], reps)
        query(ql, lrec[kind])
        out[kind] = {"lasso": row(kind, t_l, t_lc, read_counts())}
        query(qf, frec[kind])
        out[kind]["footprint"] = row(kind, t_f, t_fc, read_counts())
        out[kind]["lasso_over_footprint"] = round(t_l[0] / t_f[0], 4)
        out[kind]["lasso_over_footprint_count_only"] = round(t_lc[0] / t_fc[0], 4)
    if "half_terrain" in out:
        out["half_terrain"]["target"] = ">= 50 % of the copy rate"
        out["half_terrain"]["target_held"] = bool(out["half_terrain"]["lasso"]["frac_of_copy"] >= 0.5)
    print(json.dumps(out))


def inverse_bench(dev, u, box, st, reps, T, width, height):
    """simlod_query_inverse ALL@20 with two lassos on the screen of the camera T — the city block of --region (about 1 % of the plan area) and
    the half-terrain triangle of --footprint — each alternating rep by rep with simlod_export_octree ALL and the positive simlod_query_lasso
    ALL@20 of the same polygon, full and count-only.  An inverse is read against the export and the positive query of its own run."""
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Lasso, Region
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = max(int(L.simlod_inverse_buffer_min_bytes(nn, bound)), int(L.simlod_export_buffer_min_bytes(nn, bound)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    m = np.asarray(T, dtype=np.float64).reshape(4, 4)

    def on_screen(xy):
        h = np.concatenate([xy, np.full((len(xy), 1), 0.5 * b[2]), np.ones((len(xy), 1))], axis=1) @ m.T
        assert (h[:, 3] > 0).all()
        return np.stack([0.5 * width * (h[:, 0] / h[:, 3] + 1.0), 0.5 * height * (h[:, 1] / h[:, 3] + 1.0)], axis=1)

    tri = 0.5 + (np.array([(50 / 600, 50 / 400), (550 / 600, 80 / 400), (250 / 600, 380 / 400)]) - 0.5) * 1.25
    block = np.array([(0.45, 0.45), (0.45, 0.55), (0.55, 0.55), (0.55, 0.45)])
    plan = {"city_block": block * b[:2], "half_terrain": tri * b[:2]}
    lrec = {k: Lasso.from_pixels(T, width, height, on_screen(v)).record() for k, v in plan.items()}
    none = Region().record()

    def inverse(kind, count_only=False):
        rc = L.simlod_query_inverse(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), None, ctypes.c_void_p(lrec[kind].ctypes.data), 20,
                                    abi.EXPORT_ALL, p(scratch), ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound),
                                    p(counts), stream)
        assert rc == 0

    def positive(kind, count_only=False):
        rc = L.simlod_query_lasso(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), ctypes.c_void_p(lrec[kind].ctypes.data), 20, abi.EXPORT_ALL,
                                  p(scratch), ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def export_all():
        rc = L.simlod_export_octree(p(dev.nodes), p(dev.stats), 20, abi.EXPORT_ALL, p(scratch), ctypes.c_uint64(need), p(table), nn, p(samples),
                                    ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def read_counts():
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0].copy()
        assert int(c["error"]) == 0
        return c

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "numSamples": bound, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "screen": [width, height],
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)},
           "note": "an inverse is read against export_all and the positive lasso query of the same run"}

    def row(ms, ms_count, c):
        nbytes = int(c["numCandidates"]) * 16 + int(c["numSamples"]) * 16 + int(c["numNodes"]) * 40
        gbs = nbytes / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "count_only_ms": round(ms_count[0], 4), "nodes_listed": int(c["numNodes"]),
                "nodes_copied": int(c["numCopiedNodes"]), "nodes_filtered": int(c["numFilteredNodes"]), "numCandidates": int(c["numCandidates"]),
                "numSamples": int(c["numSamples"]), "algorithmic_bytes": nbytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4)}

    for kind in plan:
        t_inv, t_exp, t_pos, t_invc, t_posc = timed_alternating([lambda: inverse(kind), export_all, lambda: positive(kind), lambda: inverse(kind, True),
                                                                 lambda: positive(kind, True)], reps)
        inverse(kind)
        ci = read_counts()
        positive(kind)
        cp = read_counts()
        assert int(ci["numSamples"]) + int(cp["numSamples"]) == bound and int(ci["numNodes"]) == nn
        out[kind] = {"inverse": row(t_inv, t_invc, ci), "lasso": row(t_pos, t_posc, cp),
                     "export_all": {"ms": round(t_exp[0], 4), "ms_min": round(t_exp[1], 4)},
                     "removed_share": round(int(cp["numSamples"]) / bound, 4),
                     "inverse_over_export_all": round(t_inv[0] / t_exp[0], 4), "inverse_over_lasso": round(t_inv[0] / t_pos[0], 4),
                     "inverse_count_only_over_lasso_count_only": round(t_invc[0] / t_posc[0], 4)}
    print(json.dumps(out))


def rays_bench(dev, u, box, st, reps, T, width, height):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import OctreeExport, Rays, Region
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    uu, up = dev._u(u)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    b = np.asarray(box, dtype=np.float64)
    cone = Rays.from_pixels(T, width, height, [[width // 2, height // 2]], pixel_radius=0.5, t_max=3.0 * float(b.max()))
    rs = np.random.RandomState(42)
    vertical = Rays.vertical(rs.rand(4096, 2) * b[:2], b[2] + 10.0, 0.5, -10.0)
    # a thin box around the cone: four planes along the ray at its widest radius, two across it at t = 0 and tMax
    r0 = cone.record()[0]
    o, d, tmax = r0["origin"].astype(np.float64), r0["dir"].astype(np.float64), float(r0["tMax"])
    wide = float(r0["radius"]) + float(r0["spread"]) * tmax
    a1 = np.cross(d, [0.0, 0.0, 1.0]); a1 /= np.linalg.norm(a1)
    a2 = np.cross(d, a1)
    planes = [[*n, -float(n @ o) + w] for n, w in ((a1, wide), (-a1, wide), (a2, wide), (-a2, wide), (d, 0.0), (-d, tmax))]
    region = Region.from_planes(planes).record()
    q_need = int(L.simlod_query_buffer_min_bytes(nn, bound))
    q_scratch = torch.empty(q_need, dtype=torch.uint8, device=dev.device)
    q_counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)

    def region_count():
        rc = L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(region.ctypes.data), 20, abi.EXPORT_CUT, p(q_scratch),
                                   ctypes.c_uint64(q_need), p(table), nn, None, ctypes.c_uint64(0), p(q_counts), stream)
        assert rc == 0

    def setup(rays):
        d_rays = torch.from_numpy(rays.record().view(np.uint8).reshape(-1)).to(dev.device)
        n = len(rays)
        c = dev.count_rays(u, rays)
        need = int(L.simlod_rays_buffer_min_bytes(nn, bound, n, int(c["numPairs"]), int(c["numCandidates"])))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
        hits = torch.empty(n * 32, dtype=torch.uint8, device=dev.device)

        def call(count_only=False):
            rc = L.simlod_query_rays(p(dev.nodes), p(dev.stats), up, p(d_rays), n, 20, abi.EXPORT_CUT, p(scratch), ctypes.c_uint64(need), None, nn,
                                     None if count_only else p(hits), p(counts), stream)
            assert rc == 0
        return call, c, need

    cut = dev.export_octree(u, select="cut")
    n_points = int(st["numPoints"])
    copy_dst = torch.empty(n_points * 16, dtype=torch.uint8, device=dev.device)
    copy_src = cut.samples_tensor[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": n_points, "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)}}

    def counts_of(call):
        call()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.ray_counts_dtype)[0]
        assert int(c["error"]) == 0
        return {f: int(c[f]) for f in abi.ray_counts_dtype.names}

    call1, c1, need1 = setup(cone)
    t_cone, t_cone_count, t_region = timed_alternating([call1, lambda: call1(True), region_count], reps)
    torch.cuda.synchronize()
    qc = q_counts.cpu().numpy().view(abi.query_counts_dtype)[0]
    out["pixel_cone"] = {"ms": round(t_cone[0], 4), "ms_min": round(t_cone[1], 4), "count_only_ms": round(t_cone_count[0], 4), **counts_of(call1),
                         "region_count_only_ms": round(t_region[0], 4), "region_numCandidates": int(qc["numCandidates"]),
                         "over_region_count_only": round(t_cone[0] / t_region[0], 4), "target": "<= 1.5 x the count-only region query of the same run",
                         "target_held": bool(t_cone[0] <= 1.5 * t_region[0])}
    call4, c4, need4 = setup(vertical)
    t_vert, t_vert_count = timed_alternating([call4, lambda: call4(True)], reps)
    per_node = cut.rays_per_node(vertical)
    chunk_bytes = int(cut.nodes["numSamples"][per_node > 0].astype(np.int64).sum()) * 16
    ideal = chunk_bytes + len(vertical) * 32
    gbs = ideal / (t_vert[0] * 1e6)
    cv = counts_of(call4)
    gflops = cv["numCandidates"] * 25 / (t_vert[0] * 1e6)
    out["vertical_4096"] = {"ms": round(t_vert[0], 4), "ms_min": round(t_vert[1], 4), "count_only_ms": round(t_vert_count[0], 4), **cv,
                            "paired_nodes": int((per_node > 0).sum()), "distinct_chunk_bytes": chunk_bytes, "ideal_bytes": ideal, "scratch_bytes": need4,
                            "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4), "fp64_GFLOPs_at_25_per_candidate": round(gflops, 1),
                            "target": ">= 50 % of the copy rate on the ideal bytes", "target_held": bool(gbs / copy_gbs >= 0.5)}
    print(json.dumps(out))


def neighbours_bench(dev, u, box, st, reps, pts):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Rays, Spheres
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    n_q, n_mirror, target = 4096, 256, 30
    centers = pts[np.sort(np.random.RandomState(42).choice(len(pts), n_q, replace=False))]
    cut = dev.export_octree(u, select="cut").to("cpu")
    # the radius: from the surface density first, then corrected once by the mirror's median on the first queries
    radius = float(np.sqrt(target * b[0] * b[1] / (np.pi * len(pts))))
    for _ in range(2):
        within = cut.neighbours_selected(Spheres.from_points(centers[:n_mirror], radius), 1)[1]
        radius *= float(np.sqrt(target / max(float(np.median(within)), 1.0)))
    q = Spheres.from_points(centers, radius)
    mirror_within = cut.neighbours_selected(Spheres.from_records(q.record()[:n_mirror]), 1)[1]
    d_q = torch.from_numpy(q.record().view(np.uint8).reshape(-1)).to(dev.device)
    counts = torch.zeros(abi.neighbour_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    c0 = dev.count_neighbours(u, q, 16)
    need = int(L.simlod_neighbours_buffer_min_bytes(nn, bound, n_q, 16, int(c0["numPairs"]), int(c0["numCandidates"])))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    out_t = torch.empty(n_q * 16 * abi.neighbour_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    within_t = torch.empty(n_q, dtype=torch.int32, device=dev.device)

    def call(k, count_only=False):
        rc = L.simlod_query_neighbours(p(dev.nodes), p(dev.stats), up, p(d_q), n_q, k, 20, abi.EXPORT_CUT, p(scratch), ctypes.c_uint64(need), None, nn,
                                       None if count_only else p(out_t), None if count_only else p(within_t), p(counts), stream)
        assert rc == 0

    n_points = int(st["numPoints"])
    copy_dst = torch.empty(n_points * 16, dtype=torch.uint8, device=dev.device)
    copy_src = cut.samples_tensor.to(dev.device)[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": n_points, "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "queries": n_q, "radius": radius,
           "mirror_median_within": float(np.median(mirror_within)), "scratch_bytes": need,
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)}}
    ts = timed_alternating([lambda: call(1), lambda: call(8), lambda: call(16), lambda: call(16, True)], reps)
    per_node = cut.spheres_per_node(q)
    chunk_bytes = int(cut.nodes["numSamples"][per_node > 0].astype(np.int64).sum()) * 16
    for k, t in zip((1, 8, 16), ts):
        call(k)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.neighbour_counts_dtype)[0]
        assert int(c["error"]) == 0 and np.array_equal(within_t[:n_mirror].cpu().numpy().astype(np.int64), mirror_within)
        ideal = chunk_bytes + n_q * (k * 32 + 4)
        out[f"k{k}"] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), **{f: int(c[f]) for f in abi.neighbour_counts_dtype.names},
                        "ideal_bytes": ideal, "GBs": round(ideal / (t[0] * 1e6), 1), "frac_of_copy": round(ideal / (t[0] * 1e6) / copy_gbs, 4)}
    out["count_only"] = {"ms": round(ts[3][0], 4), "ms_min": round(ts[3][1], 4)}
    out["paired_nodes"], out["distinct_chunk_bytes"] = int((per_node > 0).sum()), chunk_bytes
    # for scale: the ray query's 4 096 vertical rays of radius 0.5 (export_bench --rays)
    vertical = Rays.vertical(np.random.RandomState(42).rand(4096, 2) * b[:2], b[2] + 10.0, 0.5, -10.0)
    d_rays = torch.from_numpy(vertical.record().view(np.uint8).reshape(-1)).to(dev.device)
    cr = dev.count_rays(u, vertical)
    r_need = int(L.simlod_rays_buffer_min_bytes(nn, bound, 4096, int(cr["numPairs"]), int(cr["numCandidates"])))
    r_scratch = torch.empty(r_need, dtype=torch.uint8, device=dev.device)
    hits = torch.empty(4096 * 32, dtype=torch.uint8, device=dev.device)
    r_counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)

    def rays():
        rc = L.simlod_query_rays(p(dev.nodes), p(dev.stats), up, p(d_rays), 4096, 20, abi.EXPORT_CUT, p(r_scratch), ctypes.c_uint64(r_need), None, nn,
                                 p(hits), p(r_counts), stream)
        assert rc == 0
    t_rays = timed(rays, reps)
    out["rays_vertical_4096"] = {"ms": round(t_rays[0], 4), "ms_min": round(t_rays[1], 4), "numPairs": int(cr["numPairs"]), "numCandidates": int(cr["numCandidates"])}
    print(json.dumps(out))


def compare_bench(dev, u, box, st, reps, pts, whole=False, workgroups=0, radius_arg=None, surface=False, cluster=False, align=False):
    """simlod_compare_samples: A = the CUT@20 selection of a box of 1/36 of the plan area (about 1 M samples), B = the octree's full CUT@20
    export, at --neighbours' radius of DESIGN §11 (2.167)."""
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Compare, Region, Spheres
    L, p, stream = dev.L, dev._p, dev._stream()
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    radius = 2.167 if radius_arg is None else float(radius_arg)
    side = 1.0 / 6.0
    region = Region.from_box((b[0] * (0.5 - side / 2), b[1] * (0.5 - side / 2), -1.0), (b[0] * (0.5 + side / 2), b[1] * (0.5 + side / 2), b[2] + 1.0))
    ex_b = dev.export_octree(u, 20, "cut")
    ex_a = ex_b if whole else dev.query_region(u, region, 20, "cut")
    ta, tb = ex_a.samples_tensor, ex_b.samples_tensor
    na, nb = ex_a.num_samples, ex_b.num_samples
    cmp = Compare.linear(radius, [0xFF0000FF, 0xFF00FFFF, 0xFF00FF00, 0xFFFF0000], miss_color=0xFF808080, max_workgroups=workgroups)
    pr = cmp.record(0)
    need = int(L.simlod_compare_buffer_min_bytes(na, nb))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    records = torch.empty(na * 16, dtype=torch.uint8, device=dev.device)
    colors = torch.empty(na, dtype=torch.int32, device=dev.device)
    summary = torch.zeros(abi.compare_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)

    def call(count_only=False):
        rc = L.simlod_compare_samples(up, p(ta), ctypes.c_uint64(na), p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(pr.ctypes.data), p(scratch),
                                      ctypes.c_uint64(need), None if count_only else p(records), None if count_only else p(colors), p(summary), stream)
        assert rc == 0

    copy_dst = torch.empty(nb * 16, dtype=torch.uint8, device=dev.device)
    t_copy = timed(lambda: copy_dst.copy_(tb), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    del copy_dst
    call(True)
    torch.cuda.synchronize()
    c0 = summary.cpu().numpy().view(abi.compare_summary_dtype)[0].copy()
    out = {"points": int(st["numPoints"]), "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "numA": na, "numB": nb, "radius": radius, "maxWorkgroups": workgroups, "scratch_bytes": need,
           "table_slots": int(L.simlod_compare_table_slots(nb)), "numCells": int(c0["numCells"]), "maxCellPopulation": int(c0["maxCellPopulation"]),
           "numCandidates": int(c0["numCandidates"]), "candidates_per_sample": round(int(c0["numCandidates"]) / na, 2),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * nb * 16, "GBs": round(copy_gbs, 1)}}
    if int(c0["numCandidates"]) > 4096 * na:
        out["skipped"] = "more than 4 096 candidates per sample: the call with results is not run"
        print(json.dumps(out))
        return
    ts = timed_alternating([lambda: call(), lambda: call(True)], reps)
    call()
    torch.cuda.synchronize()
    c = summary.cpu().numpy().view(abi.compare_summary_dtype)[0]
    assert int(c["error"]) == 0
    # the ideal bytes: b read once and its grid records written once and read once, a read once, a record and a colour written per sample of a
    ideal = nb * 16 * 3 + na * (16 + 16 + 4)
    ideal_test = int(c["numCandidates"]) * 16 + na * (16 + 16 + 4)
    out["results"] = {"ms": round(ts[0][0], 4), "ms_min": round(ts[0][1], 4), "ideal_bytes": ideal, "GBs": round(ideal / (ts[0][0] * 1e6), 1),
                      "frac_of_copy": round(ideal / (ts[0][0] * 1e6) / copy_gbs, 4), "numMatched": int(c["numMatched"]), "numWithin": int(c["numWithin"]),
                      "maxD2": float(c["maxD2"]), "Msamples_per_s": round(na / (ts[0][0] * 1e3), 1)}
    out["count_only"] = {"ms": round(ts[1][0], 4), "ms_min": round(ts[1][1], 4)}
    # each kernel's share: one call between the library's own events
    for name, co in (("kernels_ms", False), ("kernels_ms_count_only", True)):
        L.simlod_profile_enable(1)
        call(co)
        torch.cuda.synchronize()
        import bench
        prof = bench.collect_profile(L)
        L.simlod_profile_enable(0)
        out[name] = {k: round(ms, 4) for k, (n, ms) in prof.items() if k.startswith("k_c_")}
    if "k_c_test" in out["kernels_ms"]:
        t_test = out["kernels_ms"]["k_c_test"]
        out["test_pass"] = {"candidate_bytes": ideal_test, "GBs": round(ideal_test / (t_test * 1e6), 1),
                            "Gtests_per_s": round(int(c["numCandidates"]) / (t_test * 1e6), 2)}
    if surface:
        # simlod_surface_samples on the same two arrays at the same radius, alternating rep by rep with the compare call; its kernels from one
        # call between the library's own events (the six grid kernels are the compare call's own)
        from simlod_amd.octree_io import Surface
        sp = Surface.hillshade(radius, (1.0, 1.0, 2.0), [0xFF202020, 0xFFFFFFFF], miss_color=0xFF808080, max_workgroups=workgroups).record(0)
        s_records = torch.empty(na * abi.surface_record_dtype.itemsize, dtype=torch.uint8, device=dev.device)
        s_summary = torch.zeros(abi.surface_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)

        def scall():
            rc = L.simlod_surface_samples(up, p(ta), ctypes.c_uint64(na), p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(sp.ctypes.data), p(scratch),
                                          ctypes.c_uint64(need), p(s_records), p(colors), p(s_summary), stream)
            assert rc == 0
        tss = timed_alternating([scall, lambda: call()], reps)
        L.simlod_profile_enable(1)
        scall()
        torch.cuda.synchronize()
        import bench
        prof = bench.collect_profile(L)
        L.simlod_profile_enable(0)
        sc = s_summary.cpu().numpy().view(abi.surface_summary_dtype)[0]
        assert int(sc["error"]) == 0 and int(sc["numCandidates"]) == int(c["numCandidates"])
        kernels = {k: round(ms, 4) for k, (n, ms) in prof.items() if k.startswith("k_c_") or k.startswith("k_s_")}
        out["surface"] = {"ms": round(tss[0][0], 4), "ms_min": round(tss[0][1], 4), "compare_ms_beside_it": round(tss[1][0], 4), "kernels_ms": kernels,
                          "numEstimated": int(sc["numEstimated"]), "numDegenerate": int(sc["numDegenerate"]), "numWithin": int(sc["numWithin"]),
                          "Msamples_per_s": round(na / (tss[0][0] * 1e3), 1)}
        if "k_s_test" in kernels and "k_c_test" in out["kernels_ms"]:
            out["surface"]["k_s_test_over_k_c_test"] = round(kernels["k_s_test"] / out["kernels_ms"]["k_c_test"], 3)
    if align:
        # simlod_align_samples on the same two arrays at the same radius under a small motion: a build call and a reuse call (no records: the ICP's
        # calls), alternating rep by rep with the compare call; each call's kernels from one call between the library's own events; and a
        # 20-step DeviceOctree.register_samples (its summaries read back, its updates solved on the host) beside 20 compare calls: ONE
        # wall-clock sample each, the host's solves included, after a registration of one step that warms the scratch buffer
        import time
        import bench
        from simlod_amd.octree_io import Align
        al = Align(radius, max_candidates=0, max_workgroups=workgroups)
        centre = (b[0] * 0.5, b[1] * 0.5, b[2] * 0.5)
        ang = np.deg2rad(0.05)
        R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
        pose = np.hstack([R, (np.asarray(centre) - R @ np.asarray(centre) + np.array([0.3, -0.2, 0.1]) * radius).reshape(3, 1)])
        a_need = int(L.simlod_align_buffer_min_bytes(na, nb))
        a_scratch = torch.empty(a_need, dtype=torch.uint8, device=dev.device)
        a_summary = torch.zeros(abi.align_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)
        recs = {False: al.record(pose, 0, 0), True: al.record(pose, abi.ALIGN_REUSE_GRID, 0)}

        def acall(reuse):
            rc = L.simlod_align_samples(up, p(ta), ctypes.c_uint64(na), p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(recs[reuse].ctypes.data), p(a_scratch),
                                        ctypes.c_uint64(a_need), None, p(a_summary), stream)
            assert rc == 0
        acall(False)
        torch.cuda.synchronize()
        built = a_summary.cpu().numpy().view(abi.align_summary_dtype)[0].copy()
        tas = timed_alternating([lambda: acall(False), lambda: acall(True), lambda: call()], reps)
        acall(True)
        torch.cuda.synchronize()
        reused = a_summary.cpu().numpy().view(abi.align_summary_dtype)[0].copy()
        assert int(built["error"]) == 0 and reused.tobytes() == built.tobytes()
        kernels = {}
        for name, reuse in (("build", False), ("reuse", True)):
            L.simlod_profile_enable(1)
            acall(reuse)
            torch.cuda.synchronize()
            prof = bench.collect_profile(L)
            L.simlod_profile_enable(0)
            kernels[name] = {k: round(ms, 4) for k, (n, ms) in prof.items() if k.startswith("k_c_") or k.startswith("k_a_")}
        out["align"] = {"scratch_bytes": a_need, "build_ms": round(tas[0][0], 4), "build_ms_min": round(tas[0][1], 4), "reuse_ms": round(tas[1][0], 4),
                        "reuse_ms_min": round(tas[1][1], 4), "compare_ms_beside_it": round(tas[2][0], 4), "reuse_over_build": round(tas[1][0] / tas[0][0], 4),
                        "kernels_ms": kernels, "numMatched": int(built["numMatched"]), "numSummed": int(built["numSummed"]), "numOutside": int(built["numOutside"])}
        if "k_a_test" in kernels["reuse"] and "k_c_test" in out["kernels_ms"]:
            out["align"]["k_a_test_over_k_c_test"] = round(kernels["reuse"]["k_a_test"] / out["kernels_ms"]["k_c_test"], 3)
        dev.register_samples(u, ta, tb, al, pose=pose, iterations=1)           # (warm: the octree's shared scratch buffer grows to the size once)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = dev.register_samples(u, ta, tb, al, pose=pose, iterations=20, tol=0.0)
        torch.cuda.synchronize()
        t_reg = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t_cmp = (time.perf_counter() - t0) * 1e3
        out["align"]["register_20"] = {"steps": res.steps, "ms": round(t_reg, 3), "compare_x20_ms": round(t_cmp, 3), "over_compare_x20": round(t_reg / t_cmp, 4),
                                       "rms_first": res.rms[0] if res.rms else None, "rms_last": res.rms[-1] if res.rms else None}
    if cluster:
        # simlod_cluster_samples on A alone at the same radius, with minNeighbours 1 and 8, alternating rep by rep with simlod_compare_samples(A, A) —
        # the yardstick on the same input —; each call's kernels from one call between the library's own events
        from simlod_amd.octree_io import Cluster
        k_need = int(L.simlod_cluster_buffer_min_bytes(na))
        k_scratch = torch.empty(k_need, dtype=torch.uint8, device=dev.device)
        k_records = torch.empty(na * abi.cluster_record_dtype.itemsize, dtype=torch.uint8, device=dev.device)
        k_summary = torch.zeros(abi.cluster_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)
        a_summary = torch.zeros(abi.compare_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)
        kp = {m: Cluster(radius, m, 1, max_workgroups=workgroups).record(0) for m in (1, 8)}

        def kcall(m):
            rc = L.simlod_cluster_samples(up, p(ta), ctypes.c_uint64(na), ctypes.c_void_p(kp[m].ctypes.data), p(k_scratch), ctypes.c_uint64(k_need),
                                          p(k_records), p(colors), p(k_summary), stream)
            assert rc == 0

        def acall():
            rc = L.simlod_compare_samples(up, p(ta), ctypes.c_uint64(na), p(ta), ctypes.c_uint64(na), ctypes.c_void_p(pr.ctypes.data), p(k_scratch),
                                          ctypes.c_uint64(k_need), p(records), p(colors), p(a_summary), stream)
            assert rc == 0
        tks = timed_alternating([lambda: kcall(1), lambda: kcall(8), acall], reps)
        import bench
        out["cluster"] = {"scratch_bytes": k_need, "compare_a_a_ms": round(tks[2][0], 4), "compare_a_a_ms_min": round(tks[2][1], 4)}
        L.simlod_profile_enable(1)
        acall()
        torch.cuda.synchronize()
        prof = bench.collect_profile(L)
        L.simlod_profile_enable(0)
        out["cluster"]["compare_a_a_kernels_ms"] = {k: round(ms, 4) for k, (n, ms) in prof.items() if k.startswith("k_c_")}
        t_test = out["cluster"]["compare_a_a_kernels_ms"].get("k_c_test")
        for i, m in enumerate((1, 8)):
            L.simlod_profile_enable(1)
            kcall(m)
            torch.cuda.synchronize()
            prof = bench.collect_profile(L)
            L.simlod_profile_enable(0)
            kc = k_summary.cpu().numpy().view(abi.cluster_summary_dtype)[0]
            assert int(kc["error"]) == 0
            kernels = {k: round(ms, 4) for k, (n, ms) in prof.items() if k.startswith("k_c_") or k.startswith("k_k_")}
            row = {"ms": round(tks[i][0], 4), "ms_min": round(tks[i][1], 4), "over_compare_a_a": round(tks[i][0] / tks[2][0], 3), "kernels_ms": kernels,
                   "numClusters": int(kc["numClusters"]), "largestSize": int(kc["largestSize"]), "largestCluster": int(kc["largestCluster"]),
                   "numCore": int(kc["numCore"]), "numBorder": int(kc["numBorder"]), "numNoise": int(kc["numNoise"]), "numWithin": int(kc["numWithin"]),
                   "numCandidates": int(kc["numCandidates"]), "Msamples_per_s": round(na / (tks[i][0] * 1e3), 1)}
            if t_test and "k_k_link" in kernels and "k_k_core" in kernels:
                row["k_k_core_over_k_c_test"] = round(kernels["k_k_core"] / t_test, 3)
                row["k_k_link_over_k_c_test"] = round(kernels["k_k_link"] / t_test, 3)
            out["cluster"][f"minNeighbours_{m}"] = row
        del k_scratch, k_records
    if not whole and radius_arg is None and not surface and not cluster:
        # for scale: the same positions through simlod_query_neighbours at k = 1, in batches of 65 536 queries (each sized by its own
        # count-only call); the sum of the batches' medians of three runs is the figure
        centers = ex_a.samples
        n_q = 1 << 16
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        per_batch, candidates = [], 0
        for lo in range(0, na, n_q):
            q = Spheres.from_points(centers[lo:lo + n_q], radius)
            nq = len(q)
            d_q = torch.from_numpy(q.record().view(np.uint8).reshape(-1)).to(dev.device)
            cn = dev.count_neighbours(u, q, 1)
            n_need = int(L.simlod_neighbours_buffer_min_bytes(nn, bound, nq, 1, int(cn["numPairs"]), int(cn["numCandidates"])))
            n_scratch = torch.empty(n_need, dtype=torch.uint8, device=dev.device)
            n_out = torch.empty(nq * abi.neighbour_dtype.itemsize, dtype=torch.uint8, device=dev.device)
            n_within = torch.empty(nq, dtype=torch.int32, device=dev.device)
            n_counts = torch.zeros(abi.neighbour_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)

            def nbq():
                rc = L.simlod_query_neighbours(p(dev.nodes), p(dev.stats), up, p(d_q), nq, 1, 20, abi.EXPORT_CUT, p(n_scratch), ctypes.c_uint64(n_need), None, nn,
                                               p(n_out), p(n_within), p(n_counts), stream)
                assert rc == 0
            per_batch.append(timed(nbq, 3, warmup=1)[0])
            candidates += int(cn["numCandidates"])
            del n_scratch, n_out, n_within, d_q
        total = float(sum(per_batch))
        out["find_neighbours_k1"] = {"queries": na, "batches": len(per_batch), "ms": round(total, 2), "ms_per_batch_min": round(min(per_batch), 3),
                                     "ms_per_batch_max": round(max(per_batch), 3), "numCandidates": candidates, "candidates_per_query": round(candidates / na, 1),
                                     "Msamples_per_s": round(na / (total * 1e3), 3), "ratio_to_compare": round((na / total) / (na / ts[0][0]), 5)}
    print(json.dumps(out))


def view_bench(dev, u, box, st, reps):
    from simlod_amd import fingerprint
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = int(L.simlod_export_buffer_min_bytes(nn, bound))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(abi.view_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    x_counts = torch.zeros(16, dtype=torch.uint8, device=dev.device)
    W, H = 1920, 1080
    # bench.py's "Morro Bay - bird" and "- close" (main_progressive_octree.cpp:1314-1328), scaled to the stand-in's box
    cx, cy = 2750.218 * float(box[0]) / 6000.0, 974.775 * float(box[1]) / 4000.0
    cams = {"bird": camera.world_view_proj(camera.orbit_view(-0.207, -0.797, 3866.886 * float(box[0]) / 6000.0, (box[0] / 2, box[1] / 2, 0.35 * box[2])),
                                           camera.perspective(aspect=W / H)),
            "close": camera.world_view_proj(camera.orbit_view(-11.270, -0.225, 93.982, (cx, cy, synthetic.terrain_height(cx, cy, seed=7, box=tuple(float(v) for v in box)))),
                                            camera.perspective(aspect=W / H))}
    view = abi.view_record()
    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copy_gbs = 2 * copy_dst.numel() / (t_copy[0] * 1e6)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(copy_gbs, 1)}}
    for name, T in cams.items():
        uc = dev.uniforms(W, H, T, box, hqs=True)
        uu, up = dev._u(uc)

        def query(count_only=False):
            rc = L.simlod_query_view(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(view.ctypes.data), 20, p(scratch), ctypes.c_uint64(need), p(table), nn,
                                     None if count_only else p(samples), ctypes.c_uint64(bound), p(counts), stream)
            assert rc == 0

        def export_visible():
            rc = L.simlod_export_octree(p(dev.nodes), p(dev.stats), 20, abi.EXPORT_VISIBLE, p(scratch), ctypes.c_uint64(need), p(table), nn, p(samples),
                                        ctypes.c_uint64(bound), p(x_counts), stream)
            assert rc == 0

        def frame_and_export():
            dev.render(uc)
            export_visible()

        dev.render(uc)                                                              # the frame the VISIBLE export describes
        export_visible()
        torch.cuda.synchronize()
        xc = x_counts.cpu().numpy().view(abi.export_counts_dtype)[0].copy()
        want_t, want_s = table.clone(), samples[: int(xc["numSamples"]) * 16].clone()
        query()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.view_counts_dtype)[0].copy()
        assert int(c["error"]) == 0 and int(xc["error"]) == 0 and int(c["numSamples"]) == int(xc["numSamples"]) and int(c["numNodes"]) == int(xc["numNodes"])
        assert torch.equal(table, want_t) and torch.equal(samples[: want_s.numel()], want_s), "the view query is not the frame's VISIBLE export"
        t_view, t_vis = timed_alternating([query, export_visible], reps)
        t_count = timed(lambda: query(True), reps)
        t_path = timed(frame_and_export, reps)
        nbytes = 2 * int(c["numSamples"]) * 16 + nn * 40
        out[name] = {"ms": round(t_view[0], 4), "ms_min": round(t_view[1], 4), "export_visible_ms": round(t_vis[0], 4), "export_visible_ms_min": round(t_vis[1], 4),
                     "over_export_visible": round(t_view[0] / t_vis[0], 4), "bound": "t_view <= 1.10 * t_export_visible of the same run",
                     "bound_held": bool(t_view[0] <= 1.10 * t_vis[0]), "count_only_ms": round(t_count[0], 4), "count_only_ms_min": round(t_count[1], 4),
                     "render_plus_export_visible_ms": round(t_path[0], 4), "render_plus_export_over_view": round(t_path[0] / t_view[0], 4),
                     "numSelected": int(c["numSelected"]), "numInside": int(c["numInside"]), "numSamples": int(c["numSamples"]),
                     "samplesAt": [int(v) for v in c["samplesAt"][:12]], "algorithmic_bytes": nbytes, "GBs": round(nbytes / (t_view[0] * 1e6), 1),
                     "frac_of_copy": round(nbytes / (t_view[0] * 1e6) / copy_gbs, 4)}
    print(json.dumps(out))


def view_delta_bench(dev, u, box, st, reps, only=None):
    import math
    from simlod_amd import fingerprint
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = max(int(L.simlod_view_delta_buffer_min_bytes(nn, bound, nn)), int(L.simlod_export_buffer_min_bytes(nn, bound)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table, entries = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device), torch.empty(nn * 24, dtype=torch.uint8, device=dev.device)
    v_table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples, delta, merged = (torch.empty(bound * 16, dtype=torch.uint8, device=dev.device) for _ in range(3))
    dropped = torch.empty(nn * 4, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(abi.delta_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    v_counts = torch.zeros(abi.view_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    x_counts = torch.zeros(16, dtype=torch.uint8, device=dev.device)
    W, H = 1920, 1080
    # bench.py's "Morro Bay - bird" and "- close" (main_progressive_octree.cpp:1314-1328), scaled to the stand-in's box, as --view
    cx, cy = 2750.218 * float(box[0]) / 6000.0, 974.775 * float(box[1]) / 4000.0
    bird = lambda yaw: camera.world_view_proj(camera.orbit_view(yaw, -0.797, 3866.886 * float(box[0]) / 6000.0, (box[0] / 2, box[1] / 2, 0.35 * box[2])),
                                              camera.perspective(aspect=W / H))
    close = camera.world_view_proj(camera.orbit_view(-11.270, -0.225, 93.982, (cx, cy, synthetic.terrain_height(cx, cy, seed=7, box=tuple(float(v) for v in box)))),
                                   camera.perspective(aspect=W / H))
    view = abi.view_record()
    uu, up = dev._u(dev.uniforms(W, H, bird(-0.207), box, hqs=True))

    def query(count_only=False, uptr=up, tb=v_table, smp=samples):
        rc = L.simlod_query_view(p(dev.nodes), p(dev.stats), uptr, ctypes.c_void_p(view.ctypes.data), 20, p(scratch), ctypes.c_uint64(need), p(tb), nn,
                                 None if count_only else p(smp), ctypes.c_uint64(bound), p(v_counts), stream)
        assert rc == 0

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    t_copy = timed(lambda: copy_dst.copy_(samples[: copy_dst.numel()]), reps)
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(2 * copy_dst.numel() / (t_copy[0] * 1e6), 1)}}
    held_cams = {"same_camera": bird(-0.207), "orbit_2deg": bird(-0.207 + math.radians(2.0)), "other_preset": close, "nothing": None}
    for name, T in held_cams.items():
        if only is not None and name != only:
            continue
        if T is None:
            held_t, held_s, nh = None, None, 0
        else:
            hu, hup = dev._u(dev.uniforms(W, H, T, box, hqs=True))
            h_table, h_samples = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device), torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
            query(uptr=hup, tb=h_table, smp=h_samples)
            torch.cuda.synchronize()
            hc = v_counts.cpu().numpy().view(abi.view_counts_dtype)[0].copy()
            assert int(hc["error"]) == 0
            nh = int(hc["numNodes"])
            held_t, held_s = h_table[: nh * 40].clone(), h_samples[: int(hc["numSamples"]) * 16].clone()
            del h_table, h_samples

        def delta_call(count_only=False):
            rc = L.simlod_query_view_delta(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(view.ctypes.data), 20, None if held_t is None else p(held_t), nh, 0,
                                           p(scratch), ctypes.c_uint64(need), p(table), nn, p(entries), None if count_only else p(delta), ctypes.c_uint64(bound),
                                           p(dropped), nn, p(counts), stream)
            assert rc == 0

        def merge():
            rc = L.simlod_merge_view_delta(None if held_t is None else p(held_t), nh, None if held_s is None else p(held_s), p(table), p(entries), n_new, p(delta),
                                           p(scratch), ctypes.c_uint64(need), p(merged), ctypes.c_uint64(bound), p(x_counts), stream)
            assert rc == 0

        query()
        delta_call()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.delta_counts_dtype)[0].copy()
        vc = v_counts.cpu().numpy().view(abi.view_counts_dtype)[0].copy()
        n_new, ns = int(vc["numNodes"]), int(vc["numSamples"])
        assert int(c["view"]["error"]) == 0 and c["view"].tobytes() == vc.tobytes() and torch.equal(table[: n_new * 40], v_table[: n_new * 40])
        merge()
        torch.cuda.synchronize()
        xc = x_counts.cpu().numpy().view(abi.export_counts_dtype)[0]
        assert int(xc["error"]) == 0 and int(xc["numSamples"]) == ns and torch.equal(merged[: ns * 16], samples[: ns * 16]), "the merge is not the view"
        t_delta, t_view, t_count = timed_alternating([delta_call, query, lambda: query(True)], reps)
        t_dcount = timed(lambda: delta_call(True), reps)
        delta_call()                                                                # (the merge's inputs, as the timed calls left other bytes in scratch only)
        t_merge = timed(merge, reps)
        out[name] = {"ms": round(t_delta[0], 4), "ms_min": round(t_delta[1], 4), "view_ms": round(t_view[0], 4), "view_ms_min": round(t_view[1], 4),
                     "view_count_only_ms": round(t_count[0], 4), "over_view": round(t_delta[0] / t_view[0], 4), "over_view_count_only": round(t_delta[0] / t_count[0], 4),
                     "delta_count_only_ms": round(t_dcount[0], 4), "merge_ms": round(t_merge[0], 4), "numHeld": nh,
                     "viewSamples": ns, "deltaSamples": int(c["numDeltaSamples"]), "keptSamples": int(c["numKeptSamples"]),
                     "sent_share": round(int(c["numDeltaSamples"]) / max(ns, 1), 4),
                     "kept": int(c["numKept"]), "grown": int(c["numGrown"]), "added": int(c["numAdded"]), "dropped": int(c["numDropped"])}
    print(json.dumps(out))


def profile_bench(dev, u, box, st, reps):
    from simlod_amd import fingerprint
    from simlod_amd.octree_io import Footprint, Profile, Region
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    need = max(int(L.simlod_profile_buffer_min_bytes(nn, bound)), int(L.simlod_footprint_buffer_min_bytes(nn, bound)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    records = torch.empty(bound * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    b = np.asarray(box, dtype=np.float64)
    # five vertices across the terrain; the half-width that gives the corridor 1 % of the plan area
    line = np.array([(0.05, 0.2), (0.3, 0.8), (0.5, 0.25), (0.72, 0.85), (0.95, 0.4)]) * b[:2]
    seg = np.diff(line, axis=0)
    length = float(np.linalg.norm(seg, axis=1).sum())
    w = 0.01 * b[0] * b[1] / (2.0 * length)
    prof = Profile.from_xy(line, w)
    # the corridor's outline as a footprint: the polyline offset by w to either side with mitred bends (the set only approximately: the
    # rectangles' square ends at a bend are not a polygon of ten vertices)
    nrm = np.stack([-seg[:, 1], seg[:, 0]], axis=1) / np.linalg.norm(seg, axis=1)[:, None]
    off = [nrm[0]] + [(nrm[i - 1] + nrm[i]) / (1.0 + float(nrm[i - 1] @ nrm[i])) for i in range(1, len(seg))] + [nrm[-1]]
    outline = Footprint.from_xy(np.concatenate([line + w * np.array(off), (line - w * np.array(off))[::-1]]))
    prec, frec, none = prof.record(), outline.record(), Region().record()

    def profile(with_records=True, count_only=False):
        rc = L.simlod_query_profile(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), ctypes.c_void_p(prec.ctypes.data), 20, abi.EXPORT_CUT,
                                    p(scratch), ctypes.c_uint64(need), p(table), nn, None if count_only else p(samples), ctypes.c_uint64(bound),
                                    p(records) if with_records and not count_only else None, p(counts), stream)
        assert rc == 0

    def footprint():
        rc = L.simlod_query_footprint(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(none.ctypes.data), ctypes.c_void_p(frec.ctypes.data), 20, abi.EXPORT_CUT,
                                      p(scratch), ctypes.c_uint64(need), p(table), nn, p(samples), ctypes.c_uint64(bound), p(counts), stream)
        assert rc == 0

    def read_counts():
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0].copy()
        assert int(c["error"]) == 0
        return c

    def row(ms, c):
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "nodes_listed": int(c["numNodes"]), "nodes_copied": int(c["numCopiedNodes"]),
                "nodes_filtered": int(c["numFilteredNodes"]), "numCandidates": int(c["numCandidates"]), "numSamples": int(c["numSamples"])}

    copy_dst = torch.empty(int(st["numPoints"]) * 16, dtype=torch.uint8, device=dev.device)
    copy_src = samples[: copy_dst.numel()]
    t_rec, t_plain, t_foot = timed_alternating([lambda: profile(True), lambda: profile(False), footprint], reps)
    t_count = timed(lambda: profile(count_only=True), reps)
    t_copy = timed(lambda: copy_dst.copy_(copy_src), reps)
    copied_per_ms = copy_dst.numel() / t_copy[0]                                # bytes copied (each read once and written once) per ms
    out = {"points": int(st["numPoints"]), "numNodes": nn, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "half_width": round(w, 4),
           "polyline_length": round(length, 2),
           "d2d_copy": {"ms": round(t_copy[0], 4), "bytes": 2 * copy_dst.numel(), "GBs": round(2 * copy_dst.numel() / (t_copy[0] * 1e6), 1)}}
    profile(True)
    c = read_counts()
    out["profile_with_records"] = row(t_rec, c)
    out["profile_with_records"]["share_of_points"] = round(int(c["numSamples"]) / max(int(st["numPoints"]), 1), 5)
    out["profile_with_records"]["count_only_ms"] = round(t_count[0], 4)
    out["profile_without_records"] = row(t_plain, c)
    footprint()
    out["footprint_outline"] = row(t_foot, read_counts())
    t_records = int(c["numSamples"]) * 16 / copied_per_ms
    limit = 1.2 * (t_foot[0] + t_records)
    out["bound"] = {"what": "t(profile with records) <= 1.2 * (t(footprint of the outline) + numSamples * 16 bytes at the copy's rate), same run",
                    "records_copy_ms": round(t_records, 5), "limit_ms": round(limit, 4), "ratio": round(t_rec[0] / limit, 4), "held": bool(t_rec[0] <= limit)}
    print(json.dumps(out))


def pack_bench(dev, u, box, st, reps):
    """simlod_pack_samples / simlod_unpack_samples of the CUT@20 export beside the same run's device-to-device copy of its 16-byte samples, in
    turns; events around the bare C calls.  Algorithmic bytes: 24 per sample (16 + 8) plus the table.  Then, for scale on this host only, the
    device-to-host copy of 8 against 16 bytes per sample into pinned memory."""
    from simlod_amd import fingerprint
    L, p, stream = dev.L, dev._p, dev._stream()
    nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    ex = dev.export_octree(u, 20, "cut")
    ns = ex.num_samples
    table, samples = ex.table_tensor, ex.samples_tensor
    need = int(L.simlod_pack_buffer_min_bytes(nn, ns))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    packed = torch.empty(ns * 8, dtype=torch.uint8, device=dev.device)
    back = torch.empty(ns * 16, dtype=torch.uint8, device=dev.device)
    copy_dst = torch.empty_like(samples)
    counts = torch.zeros(abi.pack_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)

    def pack():
        rc = L.simlod_pack_samples(up, p(table), None, ex.num_nodes, p(samples), ctypes.c_uint64(ns), p(scratch), ctypes.c_uint64(need), p(packed), p(counts), stream)
        assert rc == 0

    def unpack():
        rc = L.simlod_unpack_samples(up, p(table), None, ex.num_nodes, p(packed), ctypes.c_uint64(ns), p(scratch), ctypes.c_uint64(need), p(back), p(counts), stream)
        assert rc == 0

    pack()
    c = counts.cpu().numpy().view(abi.pack_counts_dtype)[0].copy()
    assert int(c["error"]) == 0 and int(c["numSamples"]) == ns and int(c["numInexact"]) == 0 and int(c["numAlpha"]) == 0, c
    ms_pack, ms_unpack, ms_copy = timed_alternating([pack, unpack, lambda: copy_dst.copy_(samples)], reps)
    copy_gbs = 2 * ns * 16 / (ms_copy[0] * 1e6)
    b = ns * 24 + ex.num_nodes * 40

    def row(ms):
        gbs = b / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "algorithmic_bytes": b, "GBs": round(gbs, 1), "frac_of_peak": round(gbs / PEAK_GBS, 4),
                "frac_of_copy": round(gbs / copy_gbs, 4)}
    out = {"points": int(st["numPoints"]), "numNodes": ex.num_nodes, "numSamples": ns, "reps": reps, "csrc_sha16": fingerprint.csrc_sha16(), "scratch_bytes": need,
           "numClamped": int(c["numClamped"]), "pack": row(ms_pack), "unpack": row(ms_unpack),
           "d2d_copy": {"ms": round(ms_copy[0], 4), "bytes": 2 * ns * 16, "GBs": round(copy_gbs, 1), "frac_of_peak": round(copy_gbs / PEAK_GBS, 4)},
           "target": "pack and unpack >= 50 % of the copy rate"}
    host16 = torch.empty(ns * 16, dtype=torch.uint8).pin_memory()
    host8 = torch.empty(ns * 8, dtype=torch.uint8).pin_memory()
    ms16, ms8 = timed_alternating([lambda: host16.copy_(samples, non_blocking=True), lambda: host8.copy_(packed, non_blocking=True)], max(reps // 4, 3))
    out["d2h_on_this_host"] = {"ms_16B": round(ms16[0], 3), "ms_8B": round(ms8[0], 3), "GBs_16B": round(ns * 16 / (ms16[0] * 1e6), 1), "GBs_8B": round(ns * 8 / (ms8[0] * 1e6), 1)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=36_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--persistent-gb", type=int, default=16)
    ap.add_argument("--buildable", action="store_true", help="also time simlod_import_octree_buildable (grid rebuild included)")
    ap.add_argument("--region", action="store_true", help="time simlod_query_region (whole box, half the terrain, a city block) instead")
    ap.add_argument("--footprint", action="store_true", help="time simlod_query_footprint (half the terrain, a rectangle beside its four planes, two stars) instead")
    ap.add_argument("--lasso", action="store_true", help="time simlod_query_lasso (the --footprint polygons drawn on the bird camera's 1080p screen, each beside its footprint query) instead")
    ap.add_argument("--lasso-only", default=None, choices=["half_terrain", "rect", "star7", "star128"], help="--lasso: this polygon alone (a per-kernel trace of one case)")
    ap.add_argument("--inverse", action="store_true", help="time simlod_query_inverse ALL@20 (a lasso removing about a hundredth, one removing about half) beside simlod_export_octree ALL and the positive lasso query of the same polygon instead")
    ap.add_argument("--profile", action="store_true", help="time simlod_query_profile (a 5-vertex corridor over 1 % of the terrain, with and without records, beside the footprint of its outline) instead")
    ap.add_argument("--rays", action="store_true", help="time simlod_query_rays (one pixel cone, 4 096 vertical rays) instead")
    ap.add_argument("--neighbours", action="store_true", help="time simlod_query_neighbours (4 096 queries, k = 1, 8, 16, count-only) instead")
    ap.add_argument("--view", action="store_true", help="time simlod_query_view (bird and close-up cameras beside the VISIBLE export of the same frame, count-only) instead")
    ap.add_argument("--view-delta", action="store_true", help="time simlod_query_view_delta (the bird camera against four held cuts, beside simlod_query_view) instead")
    ap.add_argument("--held", default=None, choices=["same_camera", "orbit_2deg", "other_preset", "nothing"], help="--view-delta: this held cut alone (a per-kernel trace of one case)")
    ap.add_argument("--pack", action="store_true", help="time simlod_pack_samples / simlod_unpack_samples of the CUT@20 export beside the copy of its samples instead")
    ap.add_argument("--paint", action="store_true", help="time simlod_paint_region (whole box, half the terrain, a city block; SET, BLEND, SET with previous) beside the ALL@20 region query instead")
    ap.add_argument("--paint-only", default=None, metavar="REGION:MODE", help="--paint: this case alone, e.g. city_block:set (a per-kernel trace of one case)")
    ap.add_argument("--summary", action="store_true", help="time simlod_query_summary (whole box, half the terrain, a city block; the whole box in one colour) beside the ALL@20 region query and its count-only call instead")
    ap.add_argument("--summary-only", default=None, metavar="REGION", help="--summary: this case alone, e.g. whole_box or whole_box_one_colour (a per-kernel trace of one case)")
    ap.add_argument("--compare", action="store_true", help="time simlod_compare_samples (a 1 M-sample CUT@20 selection against the full CUT@20 export at radius 2.167; count-only, with results, per kernel) beside simlod_query_neighbours k = 1 instead")
    ap.add_argument("--compare-whole", action="store_true", help="--compare with A = B = the full CUT@20 export (skipped above 4 096 candidates per sample)")
    ap.add_argument("--compare-workgroups", type=int, default=0, help="--compare / --compare-whole: SimlodCompareParams.maxWorkgroups (0: the library's choice)")
    ap.add_argument("--surface", action="store_true", help="--compare / --compare-whole: also time simlod_surface_samples on the same arrays at the same radius, alternating with the compare call, with its kernels (the neighbour yardstick is then left out)")
    ap.add_argument("--cluster", action="store_true", help="--compare / --compare-whole: also time simlod_cluster_samples on A alone at the same radius with minNeighbours 1 and 8, alternating with simlod_compare_samples(A, A), with its kernels (the neighbour yardstick is then left out)")
    ap.add_argument("--align", action="store_true", help="--compare / --compare-whole: also time simlod_align_samples on the same arrays at the same radius under a small motion: a build call and a reuse call beside the compare call, k_a_test beside k_c_test, and a 20-step register_samples beside 20 compare calls")
    ap.add_argument("--compare-radius", type=float, default=None, help="--compare: another radius (heavier cells); the neighbour yardstick is then left out")
    args = ap.parse_args()
    n_points, batch = args.points, abi.MAX_BATCH_SIZE
    pts, box = synthetic.terrain(n_points, seed=7)
    dev = DeviceOctree("cuda:0", persistent_bytes=args.persistent_gb << 30, max_pixels=1920 * 1080)
    nb = (n_points + batch - 1) // batch
    ring = dev.ring.view(torch.uint8)
    for i in range(nb):
        c = pts[i * batch:(i + 1) * batch]
        ring[i * batch * 16: i * batch * 16 + len(c) * 16].copy_(torch.from_numpy(c.view(np.uint8).reshape(-1)))
    T = camera.lookat_transform((1.8 * box[0], -1.2 * box[1], 1.4 * max(box)), (0.5 * box[0], 0.5 * box[1], 0.3 * box[2]), 1920, 1080)
    u = dev.uniforms(1920, 1080, T, box)
    dev.reset(u)
    dev.batch_sizes[:nb] = torch.tensor([min(batch, n_points - i * batch) for i in range(nb)], dtype=torch.int32, device=dev.device)
    dev.publish(nb)
    dev.uploaded_host = nb
    dev.drain(u)
    st = dev.read_stats()
    nn, ns = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
    if args.region:
        return region_bench(dev, u, box, st, args.reps)
    if args.footprint:
        return footprint_bench(dev, u, box, st, args.reps)
    if args.lasso:
        return lasso_bench(dev, u, box, st, args.reps, T, 1920, 1080, args.lasso_only)
    if args.inverse:
        return inverse_bench(dev, u, box, st, args.reps, T, 1920, 1080)
    if args.profile:
        return profile_bench(dev, u, box, st, args.reps)
    if args.rays:
        return rays_bench(dev, u, box, st, args.reps, T, 1920, 1080)
    if args.neighbours:
        return neighbours_bench(dev, u, box, st, args.reps, pts)
    if args.compare or args.compare_whole:
        return compare_bench(dev, u, box, st, args.reps, pts, whole=args.compare_whole, workgroups=args.compare_workgroups, radius_arg=args.compare_radius,
                             surface=args.surface, cluster=args.cluster, align=args.align)
    if args.view:
        return view_bench(dev, u, box, st, args.reps)
    if args.view_delta:
        return view_delta_bench(dev, u, box, st, args.reps, args.held)
    if args.pack:
        return pack_bench(dev, u, box, st, args.reps)
    if args.paint:
        return paint_bench(dev, u, box, st, args.reps, args.paint_only)
    if args.summary:
        return summary_bench(dev, u, box, st, args.reps, args.summary_only)
    L = dev.L
    need = int(L.simlod_export_buffer_min_bytes(nn, ns))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
    table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples = torch.empty(ns * 16, dtype=torch.uint8, device=dev.device)
    counts = torch.zeros(16, dtype=torch.uint8, device=dev.device)
    p = dev._p
    stream = dev._stream()

    def export(ml, sel):
        rc = L.simlod_export_octree(p(dev.nodes), p(dev.stats), ml, sel, p(scratch), ctypes.c_uint64(need), p(table), nn, p(samples), ctypes.c_uint64(ns), p(counts), stream)
        assert rc == 0

    out = {"points": n_points, "numNodes": nn, "numSamples": ns, "reps": args.reps}
    ms_all = timed(lambda: export(20, abi.EXPORT_ALL), args.reps)
    c = counts.cpu().numpy().view(abi.export_counts_dtype)[0]
    assert int(c["error"]) == 0 and int(c["numSamples"]) == ns and int(c["numNodes"]) == nn
    ms_cut = timed(lambda: export(20, abi.EXPORT_CUT), args.reps)
    n_cut = int(counts.cpu().numpy().view(abi.export_counts_dtype)[0]["numSamples"])
    export(20, abi.EXPORT_ALL)
    torch.cuda.synchronize()
    dst = DeviceOctree("cuda:0", persistent_bytes=ns // 1000 * 16100 + nn * 16100 + (64 << 20), max_pixels=64 * 64)
    nbytes = ns * 16

    def imp():
        rc = L.simlod_import_octree(p(table), nn, p(samples), ctypes.c_uint64(ns), p(scratch), ctypes.c_uint64(need), p(dst.persistent),
                                    ctypes.c_uint64(dst.persistent_bytes), p(dst.nodes), p(dst.stats), stream)
        assert rc == 0
    ms_imp = timed(imp, args.reps)
    assert int(dst.read_stats()["dbg"]) == 0 and int(dst.read_stats()["numNodes"]) == nn
    ms_bld = None
    if args.buildable:
        inner = int(st["numInner"])
        grids = inner + 1 if inner else 1
        chunks = ns // 1000 + nn
        bld = DeviceOctree("cuda:0", persistent_bytes=chunks * 16032 + grids * abi.alloc_round(abi.GRID_BYTES) + (64 << 20), max_pixels=64 * 64)
        ub, ubp = bld._u(bld.uniforms(1920, 1080, T, box))

        def imp_b():
            rc = L.simlod_import_octree_buildable(ubp, p(table), nn, p(samples), ctypes.c_uint64(ns), p(scratch), ctypes.c_uint64(need), p(bld.persistent),
                                                  p(bld.nodes), p(bld.stats), p(bld.num_uploaded), p(bld.batch_sizes), stream)
            assert rc == 0
        ms_bld = timed(imp_b, args.reps)
        sb = bld.read_stats()
        assert int(sb["dbg"]) == 0 and int(sb["numNodes"]) == nn and int(sb["numVoxels"]) == int(st["numVoxels"])
        # the grid rebuild's algorithmic bytes: the leaves' points read once, every grid written once, the non-root inner grids read once
        rebuild_bytes = int(st["numPoints"]) * 16 + grids * abi.GRID_BYTES + (grids - 1) * abi.GRID_BYTES
        del bld
    copy_dst = torch.empty_like(samples)
    ms_copy = timed(lambda: copy_dst.copy_(samples), args.reps)
    copy_gbs = 2 * nbytes / (ms_copy[0] * 1e6)

    def row(ms, nsamp):
        b = 2 * nsamp * 16 + nn * 40
        gbs = b / (ms[0] * 1e6)
        return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "algorithmic_bytes": b, "GBs": round(gbs, 1),
                "frac_of_peak": round(gbs / PEAK_GBS, 4), "frac_of_copy": round(gbs / copy_gbs, 4)}
    out["export_all"] = row(ms_all, ns)
    out["export_cut20"] = row(ms_cut, n_cut)
    out["import"] = row(ms_imp, ns)
    if ms_bld is not None:
        out["import_buildable"] = row(ms_bld, ns)
        # the rebuild alone, as the difference to the render-only import (the same validation, node and copy kernels run in both)
        d = max(ms_bld[0] - ms_imp[0], 1e-6)
        gbs = rebuild_bytes / (d * 1e6)
        out["grid_rebuild"] = {"ms": round(d, 4), "algorithmic_bytes": rebuild_bytes, "GBs": round(gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4)}
    out["d2d_copy"] = {"ms": round(ms_copy[0], 4), "bytes": 2 * nbytes, "GBs": round(copy_gbs, 1), "frac_of_peak": round(copy_gbs / PEAK_GBS, 4)}
    out["target"] = "export ALL >= 50 % of the copy rate"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
