"""Clipped frames on the config-2 stand-in (bench.py's workload: 36 M-point terrain in 1 M batches, exact mode) at 1920 x 1080, the bird and the
close-up presets of bench.py, plain and HQS — each frame timed `--reps` times after a warm-up with device events around the bare C call
(simlod_launch_render), the variants of one comparison alternating rep by rep.  Prints one JSON line, with the kernel-source fingerprint.
  nothing_removed   INSIDE with zero planes (every node COPIED: the clipped kernels with nothing to test) beside the unclipped frame;
                    the target is t_clipped <= 1.10 * t_unclipped
  oblique           half the terrain (one oblique plane through the box centre): INSIDE, OUTSIDE, HIGHLIGHT beside the unclipped frame, with
                    the visible / emptied / filtered node counts of each
  replaces          the clipped INSIDE frame of the oblique half beside the path it replaces: query_region(select="all") + import_octree
                    into a second octree + render of that octree, in the same run
Per-kernel split: run it under `rocprofv3 --kernel-trace --stats -- python tools/clip_bench.py --only oblique` (a run of its own)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simlod_amd import abi, camera, fingerprint, synthetic  # noqa: E402
from simlod_amd.octree_io import Clip, Region, classify_nodes  # noqa: E402
from simlod_amd.runtime import DeviceOctree  # noqa: E402
from export_bench import timed_alternating  # noqa: E402

W, H = 1920, 1080
COLOUR = 0x00FF20E0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=36_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--persistent-gb", type=int, default=16)
    ap.add_argument("--only", choices=["nothing_removed", "oblique", "replaces"], default=None)
    args = ap.parse_args()
    n_points, batch = args.points, abi.MAX_BATCH_SIZE
    pts, box = synthetic.terrain(n_points, seed=7)
    dev = DeviceOctree("cuda:0", persistent_bytes=args.persistent_gb << 30, max_pixels=W * H)
    nb = (n_points + batch - 1) // batch
    ring = dev.ring.view(torch.uint8)
    for i in range(nb):
        c = pts[i * batch:(i + 1) * batch]
        ring[i * batch * 16: i * batch * 16 + len(c) * 16].copy_(torch.from_numpy(c.view(np.uint8).reshape(-1)))
    # bench.py's two cameras ("Morro Bay - bird" / "- close", scaled to the stand-in's box)
    T_bird = camera.world_view_proj(camera.orbit_view(-0.207, -0.797, 3866.886 * float(box[0]) / 6000.0, (box[0] / 2, box[1] / 2, 0.35 * box[2])),
                                    camera.perspective(aspect=W / H))
    cx, cy = 2750.218 * float(box[0]) / 6000.0, 974.775 * float(box[1]) / 4000.0
    T_close = camera.world_view_proj(camera.orbit_view(-11.270, -0.225, 93.982, (cx, cy, synthetic.terrain_height(cx, cy, seed=7, box=tuple(float(v) for v in box)))),
                                     camera.perspective(aspect=W / H))
    u0 = dev.uniforms(W, H, T_bird, box)
    dev.reset(u0)
    dev.batch_sizes[:nb] = torch.tensor([min(batch, n_points - i * batch) for i in range(nb)], dtype=torch.int32, device=dev.device)
    dev.publish(nb)
    dev.uploaded_host = nb
    dev.drain(u0)
    st = dev.read_stats()
    assert int(st["dbg"]) == 0
    b = np.asarray(box, dtype=np.float64)
    n = np.array([0.6, 0.8, 0.1])
    half = Region.from_planes([[*n, -float(n @ (b / 2))]])
    L, p, stream = dev.L, dev._p, dev._stream()

    def frame_of(octree, up):
        def frame():
            rc = L.simlod_launch_render(p(octree.render_buffer), up, p(octree.nodes), p(octree.colorbuffer), p(octree.stats), p(octree.frame_start), None, stream)
            assert rc == 0
        return frame

    def with_clip(clip, frame):
        """frame() under `clip`: the setter does no device work, so it stays inside the timed call as a viewer's per-frame clip would."""
        rec = clip.record() if clip is not None else None

        def run():
            assert L.simlod_context_set_clip(dev.ctx, ctypes.c_void_p(rec.ctypes.data) if rec is not None else None) == 0
            frame()
        return run

    def node_counts(clip, uniforms):
        dev.set_clip(clip)
        dev.render(uniforms)
        s = dev.read_stats()
        dev.set_clip(None)
        dev.render(uniforms)
        s0 = dev.read_stats()
        vis = dev.render_buffer[: int(s0["numVisibleNodes"]) * 152].cpu().numpy().view(abi.node_dtype)
        outside, inside = classify_nodes(clip.region.planes.astype(np.float64), vis, uniforms["boxMin"], uniforms["boxMax"])
        return {"visible": int(s["numVisibleNodes"]), "visible_unclipped": int(s0["numVisibleNodes"]), "emptied": int(s0["numVisibleNodes"]) - int(s["numVisibleNodes"]),
                "filtered": int((~outside & ~inside).sum()), "dbg": int(s["dbg"])}

    out = {"points": int(st["numPoints"]), "numNodes": int(st["numNodes"]), "reps": args.reps, "width": W, "height": H, "csrc_sha16": fingerprint.csrc_sha16()}
    for preset, T in (("bird", T_bird), ("close", T_close)):
        for hqs in (False, True):
            name = f"{preset}_{'hqs' if hqs else 'plain'}"
            uniforms = dev.uniforms(W, H, T, box, hqs=hqs)
            uu, up = dev._u(uniforms)
            frame = frame_of(dev, up)
            row = {}
            if args.only in (None, "nothing_removed"):
                t_un, t_cl = timed_alternating([with_clip(None, frame), with_clip(Clip(Region(), "inside"), frame)], args.reps)
                row["nothing_removed"] = {"unclipped_ms": round(t_un[0], 4), "clipped_ms": round(t_cl[0], 4), "ratio": round(t_cl[0] / t_un[0], 4),
                                          "bound": "t_clipped <= 1.10 * t_unclipped of the same run", "bound_held": bool(t_cl[0] <= 1.10 * t_un[0])}
            if args.only in (None, "oblique"):
                clips = {m: Clip(half, m, COLOUR) for m in ("inside", "outside", "highlight")}
                ts = timed_alternating([with_clip(None, frame)] + [with_clip(c, frame) for c in clips.values()], args.reps)
                row["oblique"] = {"unclipped_ms": round(ts[0][0], 4)}
                for (m, c), t in zip(clips.items(), ts[1:]):
                    row["oblique"][m] = {"ms": round(t[0], 4), "ms_min": round(t[1], 4), "over_unclipped": round(t[0] / ts[0][0], 4), **node_counts(c, uniforms)}
            if args.only in (None, "replaces"):
                # the path a clipped INSIDE frame replaces: the region query (every listed node's samples), the import into a second octree, its frame
                ex = dev.query_region(uniforms, half, select="all")
                nn2, ns2 = ex.num_nodes, ex.num_samples
                second = DeviceOctree("cuda:0", persistent_bytes=ns2 // 1000 * 16100 + nn2 * 16100 + (64 << 20), max_pixels=W * H)
                u2, up2 = second._u(second.uniforms(W, H, T, box, hqs=hqs))
                frame2 = frame_of(second, up2)
                nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
                need = max(int(L.simlod_query_buffer_min_bytes(nn, bound)), int(L.simlod_export_buffer_min_bytes(nn2, ns2)))
                scratch = torch.empty(need, dtype=torch.uint8, device=dev.device)
                table = torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
                samples = torch.empty(max(ns2, 1) * 16, dtype=torch.uint8, device=dev.device)
                counts = torch.zeros(32, dtype=torch.uint8, device=dev.device)
                rec = half.record()

                def round_trip():                  # the bare C calls (the counts of the region are known from the call above)
                    assert L.simlod_query_region(p(dev.nodes), p(dev.stats), up, ctypes.c_void_p(rec.ctypes.data), 20, abi.EXPORT_ALL, p(scratch), ctypes.c_uint64(need),
                                                 p(table), nn, p(samples), ctypes.c_uint64(ns2), p(counts), stream) == 0
                    assert L.simlod_import_octree(p(table), nn2, p(samples), ctypes.c_uint64(ns2), p(scratch), ctypes.c_uint64(need), p(second.persistent),
                                                  ctypes.c_uint64(second.persistent_bytes), p(second.nodes), p(second.stats), stream) == 0
                    frame2()
                t_in, t_rt = timed_alternating([with_clip(Clip(half, "inside"), frame), round_trip], args.reps)
                assert int(second.read_stats()["dbg"]) == 0 and int(second.read_stats()["numNodes"]) == nn2
                row["replaces"] = {"clipped_inside_ms": round(t_in[0], 4), "query_import_render_ms": round(t_rt[0], 4), "ratio": round(t_rt[0] / t_in[0], 2),
                                   "nodes": nn2, "samples": ns2}
                second.close()
                del second, scratch, table, samples
            dev.set_clip(None)
            out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
