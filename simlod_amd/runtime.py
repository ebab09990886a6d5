"""Host side of the MI355X SimLOD hot paths: a headless mirror of what the reference host does around its three
kernels (modules/progressive_octree/main_progressive_octree.cpp).

    initCudaProgram()   :549-642   device buffers (nodes 40 MB, momentary 300 MB, render 200 MB, ring 50 x 16 MB, ...)
    resetCUDA()         :333-361   launch `kernel`
    uploader thread     :1040-1050 H2D copy of one batch into the ring, publish batchSizes[slot], numBatchesUploaded
    updateOctree()      :364-428   launch `kernel_construct`
    renderCUDA()        :465-546   launch `kernel_render`
    stats readback      :1201      D2H copy of Stats

Everything device-side goes through the C ABI of libsimlod_hip.so (include/simlod_hip.h); torch is used for device
memory and streams only.  There is NO CPU fallback: without the compiled library or without a GPU this module
raises.
"""
import ctypes
import os

import numpy as np
import torch

from . import abi

# SIMLOD_HIP_LIB: another build of the same library (A/B measurements of two kernel variants on one GPU box, tools/)
_LIB_PATH = os.environ.get("SIMLOD_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libsimlod_hip.so")
_lib = None


class SimlodError(RuntimeError):
    pass


def lib():
    """Load libsimlod_hip.so (built by `make -C simlod_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise SimlodError(f"{_LIB_PATH} is missing: build it with `make -C simlod_amd/csrc` (no fallback path exists)")
        L = ctypes.CDLL(_LIB_PATH)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.simlod_set_node_capacity.argtypes = [u32]
        L.simlod_set_ingest_mode.argtypes = [u32]
        L.simlod_set_construct_batch_limit.argtypes = [u32]
        L.simlod_octree_image_replaced.argtypes = [vp]
        L.simlod_context_create.argtypes = [ctypes.POINTER(vp)]
        L.simlod_context_destroy.argtypes = [vp]
        L.simlod_context_attach.argtypes = [vp, vp]
        L.simlod_context_set_node_capacity.argtypes = [vp, u32]
        L.simlod_context_set_ingest_mode.argtypes = [vp, u32]
        L.simlod_context_set_construct_batch_limit.argtypes = [vp, u32]
        L.simlod_context_hint_pending_batches.argtypes = [vp, u32]
        L.simlod_upload_counter_written.argtypes = [vp, u32]
        L.simlod_context_set_knob.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        L.simlod_context_reload_env.argtypes = [vp]
        L.simlod_context_set_clip.argtypes = [vp, vp]
        L.simlod_set_clip.argtypes = [vp]
        L.simlod_context_set_trunk_mask.argtypes = [vp, u64, u64]
        L.simlod_context_construct_buffer_min_bytes.restype = u64
        L.simlod_context_construct_buffer_min_bytes.argtypes = [vp]
        L.simlod_render_framebuffer_offset.restype = u64
        L.simlod_render_buffer_bytes.restype = u64
        L.simlod_render_buffer_bytes.argtypes = [u32, u32]
        L.simlod_construct_buffer_min_bytes.restype = u64
        L.simlod_launch_reset.argtypes = [vp] * 8
        L.simlod_launch_construct.argtypes = [vp] * 11
        L.simlod_launch_construct_chain.argtypes = [vp] * 10 + [u32, vp]
        L.simlod_launch_render.argtypes = [vp] * 8
        L.simlod_launch_render_part.argtypes = [ctypes.c_uint32] + [vp] * 8
        L.simlod_render_frame_composed.argtypes = [vp] * 10
        L.simlod_render_frame_rccl.argtypes = [vp] * 9
        L.simlod_render_depth_plane_offset.restype = u64
        L.simlod_render_depth_plane_offset.argtypes = [u32, u32]
        L.simlod_render_sum_planes_offset.restype = u64
        L.simlod_render_sum_planes_offset.argtypes = [u32, u32]
        L.simlod_render_frame_layout.argtypes = [u32, u32, vp]
        L.simlod_program_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
        L.simlod_program_destroy.argtypes = [vp]
        L.simlod_program_kernel.restype = vp
        L.simlod_program_kernel.argtypes = [vp, ctypes.c_char_p]
        L.simlod_function_max_active_blocks.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.simlod_launch_cooperative.argtypes = [vp] + [ctypes.c_uint] * 7 + [vp, ctypes.POINTER(vp)]
        L.simlod_build_info.restype = ctypes.c_char_p
        L.simlod_decode_las.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double), vp, vp]
        L.simlod_decode_las_styled.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double), vp, vp, vp]
        L.simlod_launch_colorfilter.argtypes = [vp] * 6
        L.simlod_colorfilter_buffer_min_bytes.restype = u64
        L.simlod_generate_terrain.argtypes = [vp, u64, u64, u64, u32, u32, ctypes.POINTER(ctypes.c_float), vp]
        L.simlod_generate_terrain_scan.argtypes = [vp, u64, u64, u64, u32, u32, ctypes.POINTER(ctypes.c_float), ctypes.c_float, vp]
        L.simlod_export_buffer_min_bytes.restype = u64
        L.simlod_export_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_export_octree.argtypes = [vp, vp, u32, u32, vp, u64, vp, u32, vp, u64, vp, vp]
        L.simlod_import_octree.argtypes = [vp, u32, vp, u64, vp, u64, vp, u64, vp, vp, vp]
        L.simlod_import_octree_buildable.argtypes = [vp, vp, u32, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp]
        L.simlod_query_buffer_min_bytes.restype = u64
        L.simlod_query_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_region.argtypes = [vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, u64, vp, vp]
        L.simlod_footprint_buffer_min_bytes.restype = u64
        L.simlod_footprint_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_footprint.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, u64, vp, vp]
        L.simlod_paint_buffer_min_bytes.restype = u64
        L.simlod_paint_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_paint_region.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp]
        L.simlod_summary_buffer_min_bytes.restype = u64
        L.simlod_summary_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_summary.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, vp, vp]
        L.simlod_lasso_buffer_min_bytes.restype = u64
        L.simlod_lasso_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_lasso.argtypes = L.simlod_query_footprint.argtypes
        L.simlod_paint_lasso.argtypes = L.simlod_paint_region.argtypes
        L.simlod_query_summary_lasso.argtypes = L.simlod_query_summary.argtypes
        L.simlod_inverse_buffer_min_bytes.restype = u64
        L.simlod_inverse_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_inverse.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, u64, vp, vp]
        L.simlod_paint_inverse.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, u32, vp, vp, u64, vp, vp]
        L.simlod_query_summary_inverse.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, vp, vp]
        L.simlod_profile_buffer_min_bytes.restype = u64
        L.simlod_profile_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_query_profile.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, u64, vp, u32, vp, u64, vp, vp, vp]
        L.simlod_query_view.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, u32, vp, u64, vp, vp]
        L.simlod_view_delta_buffer_min_bytes.restype = u64
        L.simlod_view_delta_buffer_min_bytes.argtypes = [u32, u64, u32]
        L.simlod_query_view_delta.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, vp, u64, vp, u32, vp, vp, u64, vp, u32, vp, vp]
        L.simlod_merge_view_delta.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u64, vp, u64, vp, vp]
        L.simlod_pack_buffer_min_bytes.restype = u64
        L.simlod_pack_buffer_min_bytes.argtypes = [u32, u64]
        L.simlod_pack_samples.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, vp, vp, vp]
        L.simlod_unpack_samples.argtypes = [vp, vp, vp, u32, vp, u64, vp, u64, vp, vp, vp]
        L.simlod_rays_buffer_min_bytes.restype = u64
        L.simlod_rays_buffer_min_bytes.argtypes = [u32, u64, u32, u64, u64]
        L.simlod_query_rays.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, u64, vp, u32, vp, vp, vp]
        L.simlod_neighbours_buffer_min_bytes.restype = u64
        L.simlod_neighbours_buffer_min_bytes.argtypes = [u32, u64, u32, u32, u64, u64]
        L.simlod_query_neighbours.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, u32, vp, vp, vp, vp]
        L.simlod_compare_buffer_min_bytes.restype = u64
        L.simlod_compare_buffer_min_bytes.argtypes = [u64, u64]
        L.simlod_compare_table_slots.restype = u64
        L.simlod_compare_table_slots.argtypes = [u64]
        L.simlod_compare_samples.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp]
        L.simlod_surface_buffer_min_bytes.restype = u64
        L.simlod_surface_buffer_min_bytes.argtypes = [u64, u64]
        L.simlod_surface_samples.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp]
        L.simlod_cluster_buffer_min_bytes.restype = u64
        L.simlod_cluster_buffer_min_bytes.argtypes = [u64]
        L.simlod_cluster_samples.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]
        abi.align_prototypes(L)
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "simlod_set_node_capacity", "simlod_render_framebuffer_offset", "simlod_render_buffer_bytes",
    "simlod_construct_buffer_min_bytes", "simlod_launch_reset", "simlod_launch_construct", "simlod_launch_construct_chain", "simlod_launch_render",
    "simlod_program_create", "simlod_program_destroy", "simlod_program_kernel", "simlod_function_max_active_blocks",
    "simlod_launch_cooperative", "simlod_build_info", "simlod_decode_las", "simlod_launch_render_part",
    "simlod_render_depth_plane_offset", "simlod_render_sum_planes_offset", "simlod_render_frame_layout", "simlod_set_ingest_mode", "simlod_set_construct_batch_limit",
    "simlod_context_create", "simlod_context_destroy", "simlod_context_attach", "simlod_context_set_node_capacity", "simlod_context_set_ingest_mode",
    "simlod_context_set_construct_batch_limit", "simlod_context_set_knob", "simlod_context_reload_env", "simlod_context_construct_buffer_min_bytes",
    "simlod_octree_image_replaced", "simlod_render_frame_composed", "simlod_render_frame_rccl", "simlod_context_set_trunk_mask", "simlod_rccl_version",
    "simlod_context_hint_pending_batches", "simlod_upload_counter_written",
    "simlod_profile_enable", "simlod_profile_collect", "simlod_generate_terrain", "simlod_generate_terrain_scan", "simlod_launch_colorfilter", "simlod_colorfilter_buffer_min_bytes",
    "simlod_export_buffer_min_bytes", "simlod_export_octree", "simlod_import_octree", "simlod_import_octree_buildable",
    "simlod_query_buffer_min_bytes", "simlod_query_region", "simlod_rays_buffer_min_bytes", "simlod_query_rays",
    "simlod_neighbours_buffer_min_bytes", "simlod_query_neighbours", "simlod_footprint_buffer_min_bytes", "simlod_query_footprint",
    "simlod_context_set_clip", "simlod_set_clip", "simlod_query_view",
    "simlod_view_delta_buffer_min_bytes", "simlod_query_view_delta", "simlod_merge_view_delta",
    "simlod_decode_las_styled", "simlod_profile_buffer_min_bytes", "simlod_query_profile",
    "simlod_pack_buffer_min_bytes", "simlod_pack_samples", "simlod_unpack_samples",
    "simlod_paint_buffer_min_bytes", "simlod_paint_region",
    "simlod_summary_buffer_min_bytes", "simlod_query_summary",
    "simlod_lasso_buffer_min_bytes", "simlod_query_lasso", "simlod_paint_lasso", "simlod_query_summary_lasso",
    "simlod_inverse_buffer_min_bytes", "simlod_query_inverse", "simlod_paint_inverse", "simlod_query_summary_inverse",
    "simlod_compare_buffer_min_bytes", "simlod_compare_table_slots", "simlod_compare_samples",
    "simlod_surface_buffer_min_bytes", "simlod_surface_samples",
    "simlod_cluster_buffer_min_bytes", "simlod_cluster_samples",
    "simlod_align_buffer_min_bytes", "simlod_align_samples",
]


def _check(code, what):
    if code != 0:
        raise SimlodError(f"{what} failed with hipError {code}")


class Program:
    """CudaModularProgram look-alike (include/CudaModularProgram.h:140-264): modules -> kernels[name]."""

    def __init__(self, modules, kernels):
        L = lib()
        self._h = ctypes.c_void_p()
        m = (ctypes.c_char_p * len(modules))(*[s.encode() for s in modules])
        k = (ctypes.c_char_p * len(kernels))(*[s.encode() for s in kernels])
        _check(L.simlod_program_create(ctypes.byref(self._h), m, len(modules), k, len(kernels)), "simlod_program_create")
        self.kernels = {name: L.simlod_program_kernel(self._h, name.encode()) for name in kernels}

    def __del__(self):
        if getattr(self, "_h", None):
            lib().simlod_program_destroy(self._h)
            self._h = None


class DeviceOctree:
    """Device buffers of initCudaProgram() + the three launches, on one GPU."""

    def __init__(self, device="cuda:0", *, persistent_bytes=4 << 30, momentary_bytes=300_000_000, max_nodes=263_157,
                 ring_slots=abi.BATCH_STREAM_SIZE, max_pixels=1920 * 1080, coalesce=False, sizes_launches=True, chain=True):
        if not torch.cuda.is_available():
            raise SimlodError("no GPU visible: the SimLOD hot paths only exist as gfx950 kernels")
        self.L = lib()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.max_nodes = max_nodes
        self._layouts = {}                 # frame_layout's records by (W, H)
        # this octree's own context (include/simlod_hip.h): node capacity, ingest granularity — exact = the reference's batch-by-batch
        # bookkeeping; coalesced = all pending batches of a launch as one (same octree content, different allocator / chunk-pool
        # counters) —, batch limit, tuning knobs (from the environment as it is NOW), second stream; launches find it by the node array
        ctx = ctypes.c_void_p()
        _check(self.L.simlod_context_create(ctypes.byref(ctx)), "simlod_context_create")
        self.ctx = ctx
        _check(self.L.simlod_context_set_node_capacity(ctx, max_nodes), "simlod_context_set_node_capacity")
        _check(self.L.simlod_context_set_ingest_mode(ctx, 1 if coalesce else 0), "simlod_context_set_ingest_mode")
        self.batch_limit = abi.MAX_BATCHES_PER_LAUNCH
        # How many batches a launch can find.  Every write of the upload counter goes past the library (publish -> simlod_upload_counter_written), as
        # shim/cuda.h does with the cuMemsetD32Async of the reference's uploader (main_progressive_octree.cpp:1047-1050): the library sizes its launches
        # by that and by what its earlier launches reported — the unchanged reference host gets the same.  sizes_launches=False: a host that tells
        # nothing (the library predicts from its launches' reports alone).  SIMLOD_HOST_HINT=1: drain() / stream() also say how many batches are
        # pending in front of every launch (simlod_context_hint_pending_batches): the two must give the same rates (bench.py reports both).
        self.notifies = sizes_launches
        # drain() enqueues the launches of a round as ONE chain (simlod_launch_construct_chain: the builder's pipeline stays full across the launch
        # boundaries).  chain=False or SIMLOD_CHAIN=0: launch by launch, as the reference host does.
        self.chain = bool(chain) and os.environ.get("SIMLOD_CHAIN", "1") != "0"
        self.hint_pending = sizes_launches and os.environ.get("SIMLOD_HOST_HINT", "0") == "1"
        z = dict(dtype=torch.uint8, device=self.device)
        # H11: the reference renders before any reset and relies on fresh VRAM reading as zero
        self.nodes = torch.zeros(max_nodes * 152, **z)
        _check(self.L.simlod_context_attach(ctx, self._p(self.nodes)), "simlod_context_attach")
        self.stats = torch.zeros(112, **z)
        self.persistent = torch.empty(persistent_bytes, **z)
        self.persistent[:1 << 20].zero_()
        self.momentary = torch.empty(momentary_bytes, **z)
        self.momentary[:1 << 20].zero_()
        self.ring_slots = ring_slots
        self.ring = torch.empty(ring_slots * abi.MAX_BATCH_SIZE * 16, **z)
        self.batch_sizes = torch.zeros(abi.BATCH_STREAM_SIZE, dtype=torch.int32, device=self.device)
        self.num_uploaded = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.frame_start = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.render_buffer = torch.empty(int(self.L.simlod_render_buffer_bytes(max_pixels, 1)), **z)
        self.colorbuffer = torch.zeros(max_pixels, dtype=torch.int32, device=self.device)
        self.las_stage = None
        self.persistent_bytes, self.momentary_bytes = persistent_bytes, momentary_bytes
        self.uploaded_host = 0
        self.processed_host = 0
        self.upload_stream = torch.cuda.Stream(device=self.device)

    def close(self):
        """Give the context back (waits for its second stream).  The buffers go with the object."""
        ctx, self.ctx = getattr(self, "ctx", None), None
        if ctx is not None and torch.cuda.is_available():
            torch.cuda.synchronize(self.device)
            self.L.simlod_context_attach(None, self._p(self.nodes))
            self.L.simlod_context_destroy(ctx)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tune(self, name, value=None):
        """Override one tuning knob of THIS octree's context (name as in the environment, e.g. "SIMLOD_OVERLAP_TAIL"); None: built-in default."""
        _check(self.L.simlod_context_set_knob(self.ctx, name.encode(), int(value or 0), 0 if value is None else 1), f"simlod_context_set_knob({name})")

    def reload_env(self):
        """Read the tuning knobs from the environment again (they are read once, when the context is made)."""
        _check(self.L.simlod_context_reload_env(self.ctx), "simlod_context_reload_env")

    def set_clip(self, clip):
        """The clip of THIS octree's frames from now on (simlod_context_set_clip; octree_io.Clip): render, render_part and render_composed
        honour it, nothing is copied.  None, or a clip of mode "off": no clip."""
        rec = clip.record() if clip is not None else None
        _check(self.L.simlod_context_set_clip(self.ctx, ctypes.c_void_p(rec.ctypes.data) if rec is not None else None), "simlod_context_set_clip")

    def set_trunk_mask(self, lo, hi):
        """Multi-GPU jobs: the nodes of levels 0-2 that split whatever this rank holds under them (simlod_context_set_trunk_mask; the mask
        comes from distributed.trunk_mask).  Takes effect with the next batch ingested — flush_trunk() ingests an empty one."""
        _check(self.L.simlod_context_set_trunk_mask(self.ctx, ctypes.c_uint64(int(lo)), ctypes.c_uint64(int(hi))), "simlod_context_set_trunk_mask")

    def flush_trunk(self, uniforms):
        """Apply a trunk mask set (or widened) after the last batch: a batch of zero points goes through the ring."""
        self.upload(np.zeros(0, dtype=abi.point_dtype))
        self.drain(uniforms)

    def set_batch_limit(self, max_batches):
        self.batch_limit = max(1, min(int(max_batches), abi.MAX_BATCHES_PER_LAUNCH))
        _check(self.L.simlod_context_set_construct_batch_limit(self.ctx, max_batches), "simlod_context_set_construct_batch_limit")

    def _hint(self, pending=None, launches=1):
        """Tell the library how many batches are pending for the next launch — or chain of `launches` — (SIMLOD_HOST_HINT=1 only; None: nothing to say)."""
        if self.hint_pending and pending is not None:
            _check(self.L.simlod_context_hint_pending_batches(self.ctx, max(0, min(int(pending), launches * self.batch_limit))), "simlod_context_hint_pending_batches")

    # -- helpers ---------------------------------------------------------------------------------------------
    def uniforms(self, width, height, transform, box_size, **kw):
        return abi.make_uniforms(width, height, transform, box_size, persistent_capacity=self.persistent_bytes,
                                 momentary_capacity=self.momentary_bytes, **kw)

    @staticmethod
    def _u(uniforms):
        u = np.ascontiguousarray(uniforms).reshape(1)
        return u, ctypes.c_void_p(u.ctypes.data)

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _p(self, t):
        return ctypes.c_void_p(t.data_ptr())

    # -- the launch surface ------------------------------------------------------------------------------------
    def reset(self, uniforms):
        u, up = self._u(uniforms)
        _check(self.L.simlod_launch_reset(up, self._p(self.persistent), self._p(self.nodes), self._p(self.stats), None,
                                          self._p(self.num_uploaded), self._p(self.batch_sizes), self._stream()), "reset")
        self.uploaded_host = 0
        self.processed_host = 0

    def upload(self, points, *, stream=None):
        """One batch into the next ring slot (host numpy array or device tensor of 16-byte records)."""
        n = len(points)
        assert n <= abi.MAX_BATCH_SIZE
        slot = self.uploaded_host % abi.BATCH_STREAM_SIZE
        assert slot < self.ring_slots, "ring smaller than BATCH_STREAM_SIZE: consume before uploading more"
        dst = self.ring[slot * abi.MAX_BATCH_SIZE * 16: slot * abi.MAX_BATCH_SIZE * 16 + n * 16]
        if isinstance(points, torch.Tensor):
            dst.copy_(points.reshape(-1).view(torch.uint8), non_blocking=True)
        else:
            dst.copy_(torch.from_numpy(np.ascontiguousarray(points).view(np.uint8).reshape(-1)), non_blocking=True)
        self.batch_sizes[slot] = n
        self.uploaded_host += 1
        self.publish(self.uploaded_host)

    def publish(self, num_batches):
        """The upload counter: `num_batches` ring batches are complete (in stream order behind their copies and their batchSizes entries), and the
        library is told so (main_progressive_octree.cpp:1047-1050 + shim/cuda.h: cuMemsetD32Async(cptr_numBatchesUploaded, ...))."""
        self.num_uploaded.fill_(num_batches)
        if self.notifies:
            _check(self.L.simlod_upload_counter_written(self._p(self.num_uploaded), int(num_batches)), "simlod_upload_counter_written")

    def upload_las(self, records, header, translation, style=None):
        """One batch of RAW LAS point records (uint8 host array or device tensor) into the next ring slot, decoded on the
        device (simlod_decode_las); translation = -boxMin as at main_progressive_octree.cpp:868.  style (a lasio.Style): the colour from
        that attribute (simlod_decode_las_styled); an elevation window is given in the file's world units and shifted by translation[2] here."""
        from . import lasio
        bpp = int(header.bytesPerPoint)
        raw = records if isinstance(records, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(records).reshape(-1))
        n = raw.numel() // bpp
        assert n <= abi.MAX_BATCH_SIZE
        slot = self.uploaded_host % abi.BATCH_STREAM_SIZE
        assert slot < self.ring_slots, "ring smaller than BATCH_STREAM_SIZE: consume before uploading more"
        if self.las_stage is None or self.las_stage.numel() < raw.numel():
            self.las_stage = torch.empty(max(raw.numel(), 1 << 20), dtype=torch.uint8, device=self.device)
        self.las_stage[: raw.numel()].copy_(raw.reshape(-1).view(torch.uint8), non_blocking=True)
        scale = (ctypes.c_double * 3)(*header.scale)
        offset = (ctypes.c_double * 3)(*lasio.decode_offset(header, translation))
        dst = self.ring.data_ptr() + slot * abi.MAX_BATCH_SIZE * 16
        if style is None:
            _check(self.L.simlod_decode_las(self._p(self.las_stage), ctypes.c_uint64(n), ctypes.c_uint32(bpp), ctypes.c_uint32(int(header.format)),
                                            scale, offset, ctypes.c_void_p(dst), self._stream()), "simlod_decode_las")
        else:
            rec = style.in_frame(translation).record()
            _check(self.L.simlod_decode_las_styled(self._p(self.las_stage), ctypes.c_uint64(n), ctypes.c_uint32(bpp), ctypes.c_uint32(int(header.format)),
                                                   scale, offset, ctypes.c_void_p(rec.ctypes.data), ctypes.c_void_p(dst), self._stream()), "simlod_decode_las_styled")
        self.batch_sizes[slot] = n
        self.uploaded_host += 1
        self.publish(self.uploaded_host)

    def add_las(self, uniforms, path, translation=None, batch=abi.MAX_BATCH_SIZE, style=None):
        """Stream a LAS file through the ring: read raw bytes, decode on the device, ingest.  style: as upload_las."""
        from . import lasio
        h = lasio.load_header(path)
        t = tuple(-float(v) for v in h.min) if translation is None else translation
        for first, count in lasio.batches(h, batch):
            if self.uploaded_host - self.processed_host >= self.ring_slots:
                self.drain(uniforms)                   # (sets processed_host to what it read back)
                assert self.uploaded_host - self.processed_host < self.ring_slots, "kernel_construct left the ring full"
            self.upload_las(lasio.read_records(path, h, first, count), h, t, style)
        self.drain(uniforms)
        return h

    def colorfilter(self, uniforms):
        """colorfilter.cu's `kernel`: average voxel colours, bottom-up (simlod_launch_colorfilter); the momentary buffer is its scratch."""
        # scratch = the render buffer, not kernel_construct's momentary buffer: the builder's recycle stack lives there and has to survive
        # (the reference, whose filter call is dead code, would run it on the momentary buffer after the last batch only)
        uu = np.array(uniforms, copy=True)
        need = int(self.L.simlod_colorfilter_buffer_min_bytes())
        if self.render_buffer.numel() < need:
            self.render_buffer = torch.empty(need, dtype=torch.uint8, device=self.device)
        uu["momentaryBufferCapacity"] = self.render_buffer.numel()
        u, up = self._u(uu)
        _check(self.L.simlod_launch_colorfilter(up, self._p(self.render_buffer), self._p(self.nodes), None, self._p(self.stats), self._stream()), "colorfilter kernel")

    def generate_terrain(self, out, first_index, points_per_tile, seed, tiles_x, tile_extent, swath_width=0.0):
        """BASELINE config 4's input made on the device: points first_index .. first_index + len(out)/16 - 1 of the tiled-terrain stream
        into the uint8 device tensor `out` (simlod_generate_terrain; with swath_width > 0: in flight lines of that width, simlod_generate_terrain_scan)."""
        n = out.numel() // 16
        ext = (ctypes.c_float * 3)(*[float(v) for v in tile_extent])
        _check(self.L.simlod_generate_terrain_scan(self._p(out), ctypes.c_uint64(n), ctypes.c_uint64(first_index), ctypes.c_uint64(points_per_tile),
                                                   ctypes.c_uint32(seed), ctypes.c_uint32(tiles_x), ext, ctypes.c_float(swath_width), self._stream()), "simlod_generate_terrain_scan")

    def construct(self, uniforms):
        u, up = self._u(uniforms)
        _check(self.L.simlod_launch_construct(up, self._p(self.ring), self._p(self.momentary), self._p(self.persistent),
                                              self._p(self.nodes), self._p(self.stats), self._p(self.frame_start), None,
                                              self._p(self.num_uploaded), self._p(self.batch_sizes), self._stream()), "kernel_construct")

    def construct_chain(self, uniforms, launches):
        """`launches` consecutive kernel_construct launches with nothing between them, as ONE call (simlod_launch_construct_chain): the octree and
        Stats afterwards are those of the last; launches=1 is construct()."""
        u, up = self._u(uniforms)
        _check(self.L.simlod_launch_construct_chain(up, self._p(self.ring), self._p(self.momentary), self._p(self.persistent),
                                                    self._p(self.nodes), self._p(self.stats), self._p(self.frame_start), None,
                                                    self._p(self.num_uploaded), self._p(self.batch_sizes), int(launches), self._stream()), "kernel_construct (chain)")

    def _launch_frame(self, uniforms, launch, what):
        """One kernel_render-shaped call: the two buffers grown to what the uniforms' W x H frame needs, then launch(the eight arguments).  -> (W, H), which the readers below take as the last frame's size"""
        u, up = self._u(uniforms)
        W, H = int(u["width"][0]), int(u["height"][0])
        need = int(self.L.simlod_render_buffer_bytes(W, H))
        if self.render_buffer.numel() < need:
            self.render_buffer = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.colorbuffer.numel() < W * H:
            self.colorbuffer = torch.zeros(W * H, dtype=torch.int32, device=self.device)
        _check(launch(self._p(self.render_buffer), up, self._p(self.nodes), self._p(self.colorbuffer), self._p(self.stats), self._p(self.frame_start), None, self._stream()), what)
        self._frame_size = W, H
        return self._frame_size

    def render(self, uniforms):
        return self._launch_frame(uniforms, self.L.simlod_launch_render, "kernel_render")

    def select_frame(self, k):
        """Switch between render buffers (distributed.render_frames_pipelined keeps two frames in flight: while the planes of one are being
        reduced across ranks, the next is rasterised into the other buffer).  Buffer 0 is the one the object was made with."""
        frames = self.__dict__.setdefault("_frames", {0: None})
        cur = self.__dict__.get("_frame", 0)
        frames[cur] = (self.render_buffer, self.colorbuffer, getattr(self, "_frame_size", None))
        if frames.get(k) is None:
            frames[k] = (torch.empty_like(self.render_buffer), torch.zeros_like(self.colorbuffer), None)
        self.render_buffer, self.colorbuffer, self._frame_size = frames[k]
        self._frame = k

    # -- a frame in parts, for composition across GPUs (simlod_launch_render_part; driven by distributed.render_frame) ----------
    def render_part(self, uniforms, part):
        self._launch_frame(uniforms, lambda *args: self.L.simlod_launch_render_part(ctypes.c_uint32(part), *args), "kernel_render part")

    REDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p)

    def render_composed(self, uniforms, reduce=None, rccl_comm=None):
        """One frame through simlod_render_frame_composed / simlod_render_frame_rccl (include/simlod_hip.h): the four parts of kernel_render with
        a reduction of the named plane over all ranks in between — `reduce(plane, data_ptr, count, elem_bytes, op, stream) -> int`, or an
        ncclComm_t as an integer address."""
        if rccl_comm is not None:
            self._launch_frame(uniforms, lambda *args: self.L.simlod_render_frame_rccl(*args, ctypes.c_void_p(rccl_comm)), "simlod_render_frame_rccl")
        else:
            cb = self.REDUCE_FN(lambda user, plane, data, count, eb, op, stream: int(reduce(plane, data, count, eb, op, stream))) if reduce is not None else None
            self._launch_frame(uniforms, lambda *args: self.L.simlod_render_frame_composed(*args, ctypes.cast(cb, ctypes.c_void_p) if cb is not None else None, None), "simlod_render_frame_composed")

    def frame_layout(self, W, H):
        """Where everything lies in the render buffer for a W x H frame: the abi.frame_layout_dtype record of simlod_render_frame_layout."""
        if (W, H) not in self._layouts:
            rec = np.zeros(1, dtype=abi.frame_layout_dtype)
            _check(self.L.simlod_render_frame_layout(W, H, ctypes.c_void_p(rec.ctypes.data)), "simlod_render_frame_layout")
            self._layouts[(W, H)] = {n: int(rec[n][0]) for n in abi.frame_layout_dtype.names}
        return self._layouts[(W, H)]

    def _plane(self, name, elem_bytes, dtype):
        W, H = self._frame_size
        off = self.frame_layout(W, H)[name]
        return self.render_buffer[off: off + W * H * elem_bytes].view(dtype)

    def _counter(self, name):
        """Counter `name` (abi.COUNTERS) of the last frame as a one-element device view."""
        lay = self.frame_layout(*self._frame_size)
        off = lay["counters"] + abi.COUNTERS[name] * lay["counterStride"]
        return self.render_buffer[off: off + 4].view(torch.int32)

    def _work_word(self, name, W, H):
        """Work word `name` (abi.WORK_WORDS) of the last W x H frame as a one-element device view."""
        off = self.frame_layout(W, H)["work"] + abi.WORK_WORDS[name] * 4
        return self.render_buffer[off: off + 4].view(torch.int32)

    def depth_plane(self):
        """The HQS depth plane as an int32 view (positive float bits: integer MIN == float MIN)."""
        return self._plane("depth", 4, torch.int32)

    def sum_planes(self):
        """{R, G, B, count} per pixel as an int32 view."""
        return self._plane("sums", 16, torch.int32)

    def framebuffer_words(self):
        """depth|colour words as an int64 view (the sign bit is never set)."""
        return self._plane("framebuffer", 8, torch.int64)

    def visible_records(self):
        """(bytes of the visible-node array, number of visible nodes of the last frame as a device tensor — no host sync)."""
        off = abi.stats_dtype.fields["numVisibleNodes"][1]
        return self.render_buffer, self.stats[off: off + 4].view(torch.int32)

    def visible_records_early(self):
        """As visible_records, but the count comes from the frame's own counter (valid once part 0 of the frame has run, clamped by the
        consumer): the all-gather of the visible nodes can be issued right behind part 0 and overlap the rest of the frame."""
        return self.render_buffer, self._counter("C_VISIBLE")

    def lists_read_through_table(self):
        """How many chunk lists the last frame's r_visible read through the builder's chunk table instead of chasing `next`."""
        return int(self._counter("C_TABLE_LISTS").item())

    def samples_outside_tiles(self):
        """How many samples the last frame's first draw pass sent down the global-atomic path — outside their draw item's LDS tile, or drawn
        without one."""
        return int(self._counter("C_OUTSIDE_TILES").item())

    def samples_binned(self, width, height):
        """How many samples the last frame's first draw pass sorted into the screen bins (r_overflow rasterises them)."""
        return int(self._work_word("W_BINNED", width, height).item())

    def draw_items(self, W, H):
        """The draw items of the last W x H frame, all size classes, as a host array of abi.draw_item_dtype (tools/raster_items.py, raster_big.py)."""
        lay = self.frame_layout(W, H)
        work = self.render_buffer[lay["work"]: lay["work"] + abi.WORK_WORDS["W_COUNT"] * 4].cpu().numpy().view(np.uint32)
        size, cap = lay["drawItemBytes"], lay["maxDrawItems"]
        return np.concatenate([self.render_buffer[lay["items"] + cl * cap * size: lay["items"] + (cl * cap + min(int(work[abi.WORK_WORDS["W_ITEMS0"] + cl]), cap)) * size]
                               .cpu().numpy().view(abi.draw_item_dtype) for cl in range(lay["itemClasses"])])

    # -- readback ------------------------------------------------------------------------------------------------
    def read_stats(self):
        return self.stats.cpu().numpy().view(abi.stats_dtype)[0].copy()

    def framebuffer(self, W, H):
        off = self.frame_layout(W, H)["framebuffer"]
        return self.render_buffer[off: off + W * H * 8].cpu().numpy().view(np.uint64).copy()

    def color(self, W, H):
        return self.colorbuffer[: W * H].cpu().numpy().view(np.uint32).copy()

    def processed(self):
        """Stats.batchletIndex as the host sees it after the stream drained (main_progressive_octree.cpp:1201-1216)."""
        torch.cuda.current_stream().synchronize()
        self.processed_host = int(self.stats[76:80].cpu().numpy().view(np.uint32)[0])
        return self.processed_host

    # kernel_construct's control block at byte 0 of the momentary buffer (csrc/construct_state.inc, struct Ctl; construct.hip asserts the offsets)
    CTL_GROUP_MAX = 44          # Ctl.groupMax (uint32): batches per group the latest launch aimed at (1: one group of kernels per batch)
    CTL_GROUPS = 184            # Ctl.expandNs[4] (uint64): groups of batches ingested since the word was last zeroed (bench.py reads it too)

    def groups_ingested(self, zero=False):
        """How many groups of batches kernel_construct has ingested since the counter was last zeroed (waits for the stream); zero=True: zero it
        (in stream order, e.g. right behind a reset — a reset does not)."""
        w = self.momentary[self.CTL_GROUPS: self.CTL_GROUPS + 8]
        if zero:
            w.zero_()
            return 0
        return int(w.cpu().numpy().view(np.uint64)[0])

    def group_size(self):
        """Batches per group the latest kernel_construct launch aimed at (exact mode: SIMLOD_EXACT_GROUP as the momentary buffer's layout and
        the memory guard allow it)."""
        return int(self.momentary[self.CTL_GROUP_MAX: self.CTL_GROUP_MAX + 4].cpu().numpy().view(np.uint32)[0])

    def drain(self, uniforms, max_launches=1000):
        """Launch kernel_construct until every uploaded batch is ingested.  One launch takes at most 20 batches and stops
        early once it has run for 10 ms (progressive_octree_voxels.cu:883, :939-949) — the reference host simply launches
        again next frame; so does this loop.  Returns the number of launches.
        With chain=True (the default) the launches of a round go to the library as ONE chain (construct_chain).  The arithmetic and the return value
        stay what they are: the number of <= 20-batch launches the chains stand for — launch counts asserted or reported anywhere stay comparable."""
        launches = 0
        idle = 0
        before = self.processed_host              # (what the host last saw: 0 after a reset; too low only costs a launch that exits at once)
        while before < self.uploaded_host and launches < max_launches:
            # as many launches as the pending batches need at 20 per launch, enqueued back to back (the reference's frame loop does not wait
            # for a launch either before it enqueues the next frame's); then ONE look at Stats
            need = -(-(self.uploaded_host - before) // self.batch_limit)
            if self.chain and need > 1:
                self._hint(self.uploaded_host - before, need)
                self.construct_chain(uniforms, need)
            else:
                for k in range(need):
                    self._hint(self.uploaded_host - before - k * self.batch_limit)
                    self.construct(uniforms)
            self._hint()
            launches += need
            after = self.processed()
            idle, before = (idle + 1 if after == before else 0), after
            # (one round without progress is no stall: a library that sizes its launches by what earlier launches REPORTED may enqueue nothing until
            # the first report of a new burst is in — include/simlod_hip.h, launch sizing)
            if idle >= 3:
                st = self.read_stats()
                raise SimlodError(f"kernel_construct made no progress (Stats.dbg={int(st['dbg']):#x}, "
                                  f"memCapacityReached={int(st['memCapacityReached'])})")
        return launches

    def stream(self, uniforms, source, num_points, batch=abi.MAX_BATCH_SIZE):
        """Feed `num_points` 16-byte records that are RESIDENT on the device (`source`: uint8 tensor) through the ring the way the reference
        host does (main_progressive_octree.cpp:1005-1050, :364-428): an uploader fills free ring slots on its own stream — copy, then
        batchSizes[slot], then numBatchesUploaded, in stream order — but never runs more than a ring ahead of what the host has seen
        processed (back-pressure, :1012); every frame launches kernel_construct once (<= 20 batches, <= 10 ms) and reads Stats back.
        Returns the number of launches.  Arbitrarily long inputs go through 50 slots."""
        nb = (num_points + batch - 1) // batch
        if self.processed() < self.uploaded_host:      # batches uploaded earlier and not yet ingested: the back-pressure below counts from an empty ring
            self.drain(uniforms)
            assert self.processed_host == self.uploaded_host, "kernel_construct left batches pending"
        base = self.uploaded_host
        src = source.reshape(-1)
        uploaded, processed, launches, stalls = 0, 0, 0, 0

        def top_up():
            # the uploader: runs of free ring slots, each run one copy (a run ends where the ring wraps or the batches stop being full), then the
            # run's batchSizes, then the counter — in stream order on the upload stream, as main_progressive_octree.cpp:1020-1050 publishes them
            nonlocal uploaded
            if uploaded >= nb or uploaded - processed >= self.ring_slots:
                return
            with torch.cuda.stream(self.upload_stream):
                while uploaded < nb and uploaded - processed < self.ring_slots:
                    slot = (base + uploaded) % abi.BATCH_STREAM_SIZE
                    assert slot < self.ring_slots, "ring smaller than BATCH_STREAM_SIZE"
                    run = min(nb - uploaded, self.ring_slots - (uploaded - processed), abi.BATCH_STREAM_SIZE - slot, self.ring_slots - slot)
                    if batch != abi.MAX_BATCH_SIZE or (uploaded + run) * batch > num_points:
                        run = 1                   # (short batches do not lie back to back in the ring)
                    n = min(run * batch, num_points - uploaded * batch)
                    self.ring[slot * abi.MAX_BATCH_SIZE * 16: slot * abi.MAX_BATCH_SIZE * 16 + n * 16].copy_(src[uploaded * batch * 16: uploaded * batch * 16 + n * 16], non_blocking=True)
                    self.batch_sizes[slot: slot + run].fill_(min(batch, n))
                    uploaded += run
                    self.publish(base + uploaded)

        self.upload_stream.wait_stream(torch.cuda.current_stream())     # (a reset enqueued just before zeroes batchSizes: the uploader starts behind it)
        top_up()
        while processed < nb:
            self.uploaded_host = base + uploaded
            self._hint(uploaded - processed)
            self.construct(uniforms)              # takes what has been published by now (k_begin reads the counter with a device-scope load)
            launches += 1
            top_up()                              # ... and the uploader refills behind it while it runs
            before, processed = processed, self.processed() - base
            if processed != before:
                stalls = 0
                continue
            # nothing taken: either nothing had been published yet (the uploader is behind: wait for it, once) or the builder refuses
            stalls += 1
            self.upload_stream.synchronize()
            if stalls > 3:
                st = self.read_stats()
                raise SimlodError(f"kernel_construct made no progress (Stats.dbg={int(st['dbg']):#x}, memCapacityReached={int(st['memCapacityReached'])})")
        self._hint()
        self.uploaded_host = base + uploaded
        self.processed_host = self.uploaded_host
        return launches

    def add_points(self, uniforms, points, batch=abi.MAX_BATCH_SIZE):
        """Upload `points` batch by batch; ingest whenever the ring would overflow and at the end."""
        for i in range(0, len(points), batch):
            if self.uploaded_host - self.processed_host >= self.ring_slots:
                self.drain(uniforms)
                assert self.uploaded_host - self.processed_host < self.ring_slots, "kernel_construct left the ring full"
            self.upload(points[i:i + batch])
        self.drain(uniforms)

    def upload_image(self, nodes, persistent, num_nodes, stats=None):
        """Load an octree image whose pointers were already rewritten for THIS object's device buffers (self.nodes.data_ptr(),
        self.persistent.data_ptr()) — e.g. one built by another implementation.  Only what kernel_render needs is set."""
        assert num_nodes <= self.max_nodes and persistent.size <= self.persistent.numel()
        self.nodes[: num_nodes * 152].copy_(torch.from_numpy(nodes[:num_nodes].view(np.uint8).reshape(-1)))
        self.persistent[: persistent.size].copy_(torch.from_numpy(persistent))
        st = np.zeros(1, dtype=abi.stats_dtype) if stats is None else np.array(stats, dtype=abi.stats_dtype).reshape(1).copy()
        st["numNodes"] = num_nodes
        self.stats.copy_(torch.from_numpy(st.view(np.uint8).reshape(-1)))
        self.momentary[:4096].zero_()          # control block: the builder's side tables describe the previous octree
        _check(self.L.simlod_octree_image_replaced(self.nodes.data_ptr()), "simlod_octree_image_replaced")
        self.processed_host = int(st["batchletIndex"][0])

    # -- export / import (include/simlod_hip.h, "octree export / import"; simlod_amd/octree_io.py) ----------------------------------------
    def _export_scratch(self, need):
        t = self.__dict__.get("_xscratch")
        if t is None or t.numel() < need:
            t = self._xscratch = torch.empty(max(int(need), 1 << 20), dtype=torch.uint8, device=self.device)
        return t

    def export_octree(self, uniforms, max_level=None, select="all"):
        """The octree as an octree_io.OctreeExport on this device: nodes with level <= max_level (None: all) and the samples of the nodes
        `select` names ("all", "cut": the leaves of the truncated table, "visible": what the last render drew).  Reads Stats once to size
        the outputs; raises SimlodError when the device reports an error."""
        from .octree_io import OctreeExport
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)
        ml = abi.MAX_DEPTH if max_level is None else max(0, min(int(max_level), abi.MAX_DEPTH))
        st = self.read_stats()
        nn, ns = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        need = int(self.L.simlod_export_buffer_min_bytes(nn, ns))
        scratch = self._export_scratch(need)
        table = torch.empty(max(nn, 1) * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)
        samples = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        counts = torch.zeros(abi.export_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        _check(self.L.simlod_export_octree(self._p(self.nodes), self._p(self.stats), ml, sel, self._p(scratch), ctypes.c_uint64(scratch.numel()),
                                           self._p(table), nn, self._p(samples), ctypes.c_uint64(ns), self._p(counts), self._stream()), "simlod_export_octree")
        c = counts.cpu().numpy().view(abi.export_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"simlod_export_octree reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples)")
        u = np.asarray(uniforms).reshape(-1)[0]
        return OctreeExport(table[: int(c["numNodes"]) * abi.export_node_dtype.itemsize], samples[: int(c["numSamples"]) * abi.point_dtype.itemsize],
                            u["boxMin"], u["boxMax"], ml, sel)

    # -- region queries (include/simlod_hip.h, "region queries") ---------------------------------------------------------------------------
    @staticmethod
    def _one_polygon(footprint, lasso):
        if footprint is not None and lasso is not None:
            raise ValueError("a lasso does not combine with a footprint in one call")

    def _query(self, uniforms, region, ml, sel, table, samples, sample_capacity, bound, footprint=None, lasso=None, invert=False):
        """One simlod_query_region call — with a footprint (an octree_io.Footprint) one simlod_query_footprint call, with a lasso (an
        octree_io.Lasso) one simlod_query_lasso call; invert: one simlod_query_inverse call with whichever polygon there is — -> the
        SimlodQueryCounts record (host).  samples None: count only."""
        self._one_polygon(footprint, lasso)
        u, up = self._u(uniforms)
        r = region.record()
        nn = table.numel() // abi.export_node_dtype.itemsize
        counts = torch.zeros(abi.query_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        tail = (self._p(table), nn, None if samples is None else self._p(samples), ctypes.c_uint64(sample_capacity), self._p(counts), self._stream())
        if invert:
            what = "simlod_query_inverse"
            f, l = (None if p is None else p.record() for p in (footprint, lasso))
            scratch = self._export_scratch(int(self.L.simlod_inverse_buffer_min_bytes(nn, bound)))
            rc = self.L.simlod_query_inverse(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data),
                                             None if f is None else ctypes.c_void_p(f.ctypes.data), None if l is None else ctypes.c_void_p(l.ctypes.data),
                                             ml, sel, self._p(scratch), ctypes.c_uint64(scratch.numel()), *tail)
        elif lasso is not None:
            what = "simlod_query_lasso"
            f = lasso.record()
            scratch = self._export_scratch(int(self.L.simlod_lasso_buffer_min_bytes(nn, bound)))
            rc = self.L.simlod_query_lasso(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(f.ctypes.data),
                                           ml, sel, self._p(scratch), ctypes.c_uint64(scratch.numel()), *tail)
        elif footprint is None:
            what = "simlod_query_region"
            scratch = self._export_scratch(int(self.L.simlod_query_buffer_min_bytes(nn, bound)))
            rc = self.L.simlod_query_region(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data), ml, sel, self._p(scratch),
                                            ctypes.c_uint64(scratch.numel()), *tail)
        else:
            what = "simlod_query_footprint"
            f = footprint.record()
            scratch = self._export_scratch(int(self.L.simlod_footprint_buffer_min_bytes(nn, bound)))
            rc = self.L.simlod_query_footprint(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(f.ctypes.data),
                                               ml, sel, self._p(scratch), ctypes.c_uint64(scratch.numel()), *tail)
        _check(rc, what)
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"{what} reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples)")
        return c

    def _query_setup(self, max_level, select):
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else int(select)
        ml = abi.MAX_DEPTH if max_level is None else max(0, min(int(max_level), abi.MAX_DEPTH))
        st = self.read_stats()
        return sel, ml, int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])

    def _table(self, nn):
        return torch.empty(max(nn, 1) * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)

    def count_region(self, uniforms, region, max_level=None, select="cut", footprint=None, lasso=None, invert=False):
        """How much of the octree lies in `region` (an octree_io.Region) at `max_level`: the SimlodQueryCounts record of a count-only
        simlod_query_region call (numNodes, numSamples, numCandidates, numFilteredNodes, numCopiedNodes).  No sample is written.
        footprint (an octree_io.Footprint): inside that extruded polygon as well, by simlod_query_footprint.
        lasso (an octree_io.Lasso, no footprint then): inside that polygon on the screen as well, by simlod_query_lasso.
        invert: how much lies OUTSIDE that selection, by simlod_query_inverse (numNodes is then the export's: nothing is culled)."""
        self._one_polygon(footprint, lasso)
        sel, ml, nn, bound = self._query_setup(max_level, select)
        return self._query(uniforms, region, ml, sel, self._table(nn), None, 0, bound, footprint, lasso, invert)

    def query_region(self, uniforms, region, max_level=None, select="cut", return_counts=False, footprint=None, lasso=None, invert=False):
        """The samples inside `region` as an octree_io.OctreeExport on this device (select abi.EXPORT_REGION): the pruned table and, in chunk-list
        order, the samples of the selected nodes ("cut": source leaves and the nodes at max_level; "all": every listed node) that pass the
        region's test.  A count-only call first, then the outputs sized exactly.  Raises SimlodError when the device reports an error.
        footprint (an octree_io.Footprint): the samples that are inside that extruded polygon as well, by simlod_query_footprint.
        lasso (an octree_io.Lasso, no footprint then): the samples inside that polygon on the screen as well, by simlod_query_lasso.
        invert: the samples that FAIL the selection's test, by simlod_query_inverse ("inverse selections"): the table is then the export's,
        unpruned, with the nodes the selection swallows whole listed empty — import_octree(result) is the octree with the selection erased."""
        from .octree_io import OctreeExport
        self._one_polygon(footprint, lasso)
        sel, ml, nn, bound = self._query_setup(max_level, select)
        c = self._query(uniforms, region, ml, sel, self._table(nn), None, 0, bound, footprint, lasso, invert)
        nn, ns = int(c["numNodes"]), int(c["numSamples"])
        table = torch.empty(nn * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)
        samples = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        c = self._query(uniforms, region, ml, sel, table, samples, ns, bound, footprint, lasso, invert)
        u = np.asarray(uniforms).reshape(-1)[0]
        ex = OctreeExport(table, samples[: int(c["numSamples"]) * abi.point_dtype.itemsize], u["boxMin"], u["boxMax"], ml, abi.EXPORT_REGION)
        return (ex, c) if return_counts else ex

    def erase_region(self, uniforms, region, footprint=None, lasso=None):
        """Delete, from this octree, the samples query_region(region, 20, "all", footprint / lasso) returns: the inverse query at level 20,
        select "all", on the device, then import_octree of its result into this octree — the frame SIMLOD_CLIP_OUTSIDE draws, made permanent.
        -> the SimlodQueryCounts record of the inverse query (numSamples: the samples that are left).  The tree keeps its shape: a node that
        lost every sample stays listed, empty.  As after any import_octree the octree is render-only until the next reset: construct() and
        colorfilter() refuse it.  What is removed is gone — run query_region with the same arguments first to keep it."""
        ex, c = self.query_region(uniforms, region, abi.MAX_DEPTH, "all", return_counts=True, footprint=footprint, lasso=lasso, invert=True)
        self.import_octree(ex)
        return c

    # -- paint regions (include/simlod_hip.h, "paint regions") -----------------------------------------------------------------------------
    def paint_region(self, uniforms, region, paint, footprint=None, colors=None, return_previous=False, lasso=None, invert=False):
        """Recolour, in the octree itself, the samples simlod_query_footprint(region, footprint, 20, "all") returns — `paint` (an
        octree_io.Paint) says how: set, blend, ramp by height, or array (then `colors`: one uint32 word per sample in the query's order, a
        tensor on this device or anything numpy takes) — by one simlod_paint_region call.  -> the SimlodQueryCounts record (numSamples: the
        number painted), and with return_previous (that record, the colour words the samples had: a uint32 tensor on this device, which an
        array paint of the same region and footprint puts back).  Raises SimlodError when the device reports an error; then nothing was
        painted.  No frame, query or ingest of this octree may be in flight on another stream.
        lasso (an octree_io.Lasso, no footprint then): the samples simlod_query_lasso(region, lasso, 20, "all") returns, by simlod_paint_lasso.
        invert: the samples simlod_query_inverse(region, footprint, lasso, 20, "all") returns — everything but the selection — by
        simlod_paint_inverse; return_previous and an array paint with invert=True again are the undo."""
        from .octree_io import Region
        self._one_polygon(footprint, lasso)
        u, up = self._u(uniforms)
        st = self.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        r, pr = (Region() if region is None else region).record(), paint.record()
        f = lasso.record() if lasso is not None else None if footprint is None else footprint.record()
        call, what = (self.L.simlod_paint_lasso, "simlod_paint_lasso") if lasso is not None else (self.L.simlod_paint_region, "simlod_paint_region")
        polygon = (None if f is None else ctypes.c_void_p(f.ctypes.data),)
        if invert:
            call, what = self.L.simlod_paint_inverse, "simlod_paint_inverse"
            polygon = (None, polygon[0]) if lasso is not None else (polygon[0], None)
        col = None
        if paint.mode == abi.PAINT_ARRAY:
            if colors is None:
                raise ValueError("an ARRAY paint needs colors")
            col = colors if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(colors, dtype=np.uint32)).view(np.int32))
            col = col.reshape(-1).contiguous().to(self.device)
            if col.element_size() != 4:
                raise ValueError("colors are 32-bit words")
        prev = torch.empty(max(bound, 1), dtype=torch.int32, device=self.device) if return_previous else None
        cap = min(t.numel() for t in (col, prev) if t is not None) if (col is not None or prev is not None) else 0
        table = self._table(nn)
        counts = torch.zeros(abi.query_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        scratch = self._export_scratch(int(self.L.simlod_paint_buffer_min_bytes(nn, bound)))
        opt = lambda t: None if t is None else self._p(t)
        _check(call(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data),
                    *polygon, ctypes.c_void_p(pr.ctypes.data), self._p(scratch),
                    ctypes.c_uint64(scratch.numel()), self._p(table), nn, opt(col), opt(prev), ctypes.c_uint64(cap), self._p(counts),
                    self._stream()), what)
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"{what} reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples); nothing was painted")
        return (c, prev[: int(c["numSamples"])]) if return_previous else c

    # -- summary queries (include/simlod_hip.h, "summary queries") -------------------------------------------------------------------------
    def summarize_region(self, uniforms, region, max_level=None, select="cut", footprint=None, z0=0.0, scale=1.0, max_workgroups=0, lasso=None,
                         invert=False):
        """What query_region(region, max_level, select, footprint=footprint) would return, summarised on the device by one simlod_query_summary
        call instead of copied out: an octree_io.Summary — the number of samples, their extent, the sums behind centroid and covariance, the
        histogram of their heights in the bins of a ramp paint with (z0, scale), and the histograms of the four colour bytes.  The octree is
        only read.  max_workgroups: 0, or a limit for the reduction's grid (the result does not depend on it).  Raises SimlodError when the
        device reports an error; then no summary was written.
        lasso (an octree_io.Lasso, no footprint then): what query_region(..., lasso=lasso) would return, by simlod_query_summary_lasso.
        invert: what query_region(..., invert=True) would return, by simlod_query_summary_inverse."""
        from .octree_io import Region, Summary
        self._one_polygon(footprint, lasso)
        u, up = self._u(uniforms)
        sel, ml, nn, bound = self._query_setup(max_level, select)
        r = (Region() if region is None else region).record()
        f = lasso.record() if lasso is not None else None if footprint is None else footprint.record()
        call, what = (self.L.simlod_query_summary_lasso, "simlod_query_summary_lasso") if lasso is not None else (self.L.simlod_query_summary, "simlod_query_summary")
        polygon = (None if f is None else ctypes.c_void_p(f.ctypes.data),)
        if invert:
            call, what = self.L.simlod_query_summary_inverse, "simlod_query_summary_inverse"
            polygon = (None, polygon[0]) if lasso is not None else (polygon[0], None)
        pr = np.zeros(1, dtype=abi.summary_params_dtype)
        pr["z0"], pr["scale"], pr["maxWorkgroups"] = z0, scale, int(max_workgroups)
        table = self._table(nn)
        counts = torch.zeros(abi.query_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        out = torch.zeros(abi.summary_dtype.itemsize, dtype=torch.uint8, device=self.device)
        scratch = self._export_scratch(int(self.L.simlod_summary_buffer_min_bytes(nn, bound)))
        _check(call(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data),
                    *polygon, ctypes.c_void_p(pr.ctypes.data), ml, sel, self._p(scratch),
                    ctypes.c_uint64(scratch.numel()), self._p(table), nn, self._p(out), self._p(counts), self._stream()), what)
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"{what} reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples); no summary was written")
        return Summary(out.cpu().numpy().view(abi.summary_dtype)[0], pr["z0"][0], pr["scale"][0])

    # -- compare queries (include/simlod_hip.h, "compare queries") -------------------------------------------------------------------------
    COMPARE_BUDGET_PER_SAMPLE = 64                                          # compare_region's default budget: candidates per sample of A

    def _samples_tensor(self, s):
        """Samples as a uint8 tensor on this device: a tensor of whole 16-byte records, an OctreeExport, or anything numpy takes."""
        if hasattr(s, "samples_tensor"):
            s = s.samples_tensor
        if not isinstance(s, torch.Tensor):
            s = torch.from_numpy(np.ascontiguousarray(np.asarray(s, dtype=abi.point_dtype)).view(np.uint8).reshape(-1))
        s = s.reshape(-1).view(torch.uint8).contiguous().to(self.device)
        if s.numel() == 0 or s.numel() % abi.point_dtype.itemsize:
            raise ValueError("samples are whole 16-byte records, at least one")
        return s

    def compare_samples(self, uniforms, a, b, compare, count_only=False, max_candidates=None):
        """One simlod_compare_samples call on two sample arrays (device tensors of 16-byte records, OctreeExports, or anything numpy takes):
        per sample of `a` the nearest sample of `b` within compare.radius.  -> (records: a uint8 tensor of abi.compare_record_dtype records,
        colors: an int32 tensor of colour words, both on this device and in a's order, and the abi.compare_summary_dtype record on the host);
        count_only: (None, None, record) — the grid's fields only (rule C7).  The call ALWAYS carries a candidate budget (rule C6):
        max_candidates if given, else compare.max_candidates, else — both None — 64 candidates per sample of `a`, compare_region's default;
        an explicit 0, here or in the Compare, is the opt-out (no limit).  A budget exceeded comes back as (None, None, record) with
        SIMLOD_COMPARE_ERR_BUDGET in the record's error field: no sample was tested, no record or colour written, and numCandidates and
        maxCellPopulation say why."""
        u, up = self._u(uniforms)
        ta, tb = self._samples_tensor(a), self._samples_tensor(b)
        na, nb = ta.numel() // abi.point_dtype.itemsize, tb.numel() // abi.point_dtype.itemsize
        budget = max_candidates if max_candidates is not None else compare.max_candidates
        pr = compare.record(self.COMPARE_BUDGET_PER_SAMPLE * na if budget is None else int(budget))
        need = int(self.L.simlod_compare_buffer_min_bytes(na, nb))
        if need == 0:
            raise ValueError("numA and numB are 1 .. 2^32 - 2")
        scratch = self._export_scratch(need)
        out = torch.zeros(abi.compare_summary_dtype.itemsize, dtype=torch.uint8, device=self.device)
        records = colors = None
        if not count_only:
            records = torch.empty(na * abi.compare_record_dtype.itemsize, dtype=torch.uint8, device=self.device)
            colors = torch.empty(na, dtype=torch.int32, device=self.device)
        opt = lambda t: None if t is None else self._p(t)
        _check(self.L.simlod_compare_samples(up, self._p(ta), ctypes.c_uint64(na), self._p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(pr.ctypes.data),
                                             self._p(scratch), ctypes.c_uint64(scratch.numel()), opt(records), opt(colors), self._p(out), self._stream()),
               "simlod_compare_samples")
        rec = out.cpu().numpy().view(abi.compare_summary_dtype)[0]
        return (None, None, rec) if int(rec["error"]) != 0 else (records, colors, rec)

    def _compare_inputs(self, uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select):
        from .octree_io import Region
        region = Region() if region is None else region
        a = self.query_region(uniforms, region, max_level, select, footprint=footprint, lasso=lasso, invert=invert)
        b = other.export_octree(uniforms, other_max_level, other_select)
        if a.num_samples == 0 or b.num_samples == 0:
            raise SimlodError(f"nothing to compare: the selection holds {a.num_samples} samples, the other octree's export {b.num_samples}")
        sel = {"region": region, "max_level": abi.MAX_DEPTH if max_level is None else int(max_level), "select": select, "footprint": footprint,
               "lasso": lasso, "invert": invert}
        return a, b, sel

    def count_compare(self, uniforms, other, region, compare, max_level=None, select="cut", footprint=None, lasso=None, invert=False,
                      other_max_level=None, other_select="cut"):
        """What compare_region would cost: the abi.compare_summary_dtype record of the count-only call (numCells, maxCellPopulation,
        numCandidates, the invalid counts) for the same arguments; no distance is computed and no budget applies."""
        a, b, _ = self._compare_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        return self.compare_samples(uniforms, a, b, compare, count_only=True, max_candidates=0)[2]

    def compare_region(self, uniforms, other, region, compare, max_level=None, select="cut", footprint=None, lasso=None, invert=False,
                       other_max_level=None, other_select="cut"):
        """Each sample of a selection of THIS octree against the nearest sample of `other` (a DeviceOctree on this device; may be this one)
        within compare.radius: A = query_region(region, max_level, select, footprint / lasso / invert), B = other.export_octree(
        other_max_level, other_select), a count-only simlod_compare_samples call, the budget check, then the call with results -> an
        octree_io.CompareResult (A, B, the records, the colours, the summary).  The budget is compare.max_candidates (None: 64 candidates per
        sample of A; 0: none); a count above it raises SimlodError naming numCandidates and maxCellPopulation — pick a smaller radius or a
        coarser cut of B.  With max_level=20, select="all" the colours are in the order paint_region's ARRAY paint takes:
        CompareResult.paint(dev, uniforms) writes them into the octree."""
        from .octree_io import CompareResult
        a, b, sel = self._compare_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        budget = self.COMPARE_BUDGET_PER_SAMPLE * a.num_samples if compare.max_candidates is None else compare.max_candidates
        c = self.compare_samples(uniforms, a, b, compare, count_only=True, max_candidates=0)[2]
        if budget != 0 and int(c["numCandidates"]) > budget:
            raise SimlodError(f"comparing {a.num_samples} samples with {b.num_samples} at radius {float(compare.radius)} would test numCandidates = "
                              f"{int(c['numCandidates'])} pairs, above the budget of {budget} (maxCellPopulation = {int(c['maxCellPopulation'])} in "
                              f"{int(c['numCells'])} cells): pick a smaller radius or a coarser cut of the other octree")
        records, colors, s = self.compare_samples(uniforms, a, b, compare, max_candidates=budget)
        if int(s["error"]) != 0:
            raise SimlodError(f"simlod_compare_samples reported error bits {int(s['error']):#x}; no record was written")
        return CompareResult(a, b, records, colors, s, compare, sel)

    # -- surface queries (include/simlod_hip.h, "surface queries") -------------------------------------------------------------------------
    def surface_samples(self, uniforms, a, b, surface, count_only=False, max_candidates=None):
        """One simlod_surface_samples call on two sample arrays (as compare_samples takes them; b may be a): per sample of `a` the plane
        through the samples of `b` within surface.radius.  -> (records: a uint8 tensor of abi.surface_record_dtype records, colors: an int32
        tensor of colour words, both on this device and in a's order, and the abi.surface_summary_dtype record on the host); count_only:
        (None, None, record).  The call ALWAYS carries a candidate budget, compare_samples' (rule C6): max_candidates if given, else
        surface.max_candidates, else 64 candidates per sample of `a`; an explicit 0 is the opt-out.  A budget exceeded comes back as
        (None, None, record) with SIMLOD_SURFACE_ERR_BUDGET in the record's error field."""
        u, up = self._u(uniforms)
        ta, tb = self._samples_tensor(a), self._samples_tensor(b)
        na, nb = ta.numel() // abi.point_dtype.itemsize, tb.numel() // abi.point_dtype.itemsize
        budget = max_candidates if max_candidates is not None else surface.max_candidates
        pr = surface.record(self.COMPARE_BUDGET_PER_SAMPLE * na if budget is None else int(budget))
        need = int(self.L.simlod_surface_buffer_min_bytes(na, nb))
        if need == 0:
            raise ValueError("numA and numB are 1 .. 2^32 - 2")
        scratch = self._export_scratch(need)
        out = torch.zeros(abi.surface_summary_dtype.itemsize, dtype=torch.uint8, device=self.device)
        records = colors = None
        if not count_only:
            records = torch.empty(na * abi.surface_record_dtype.itemsize, dtype=torch.uint8, device=self.device)
            colors = torch.empty(na, dtype=torch.int32, device=self.device)
        opt = lambda t: None if t is None else self._p(t)
        _check(self.L.simlod_surface_samples(up, self._p(ta), ctypes.c_uint64(na), self._p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(pr.ctypes.data),
                                             self._p(scratch), ctypes.c_uint64(scratch.numel()), opt(records), opt(colors), self._p(out), self._stream()),
               "simlod_surface_samples")
        rec = out.cpu().numpy().view(abi.surface_summary_dtype)[0]
        return (None, None, rec) if int(rec["error"]) != 0 else (records, colors, rec)

    def _surface_inputs(self, uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select):
        """compare_region's selection; other None: the selection against itself."""
        if other is not None:
            return self._compare_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        from .octree_io import Region
        region = Region() if region is None else region
        a = self.query_region(uniforms, region, max_level, select, footprint=footprint, lasso=lasso, invert=invert)
        if a.num_samples == 0:
            raise SimlodError("nothing to estimate: the selection holds no sample")
        sel = {"region": region, "max_level": abi.MAX_DEPTH if max_level is None else int(max_level), "select": select, "footprint": footprint,
               "lasso": lasso, "invert": invert}
        return a, a, sel

    def count_surface(self, uniforms, region, surface, other=None, max_level=None, select="cut", footprint=None, lasso=None, invert=False,
                      other_max_level=None, other_select="cut"):
        """What surface_region would cost: the abi.surface_summary_dtype record of the count-only call (numCells, maxCellPopulation,
        numCandidates, the invalid counts) for the same arguments; nothing is estimated and no budget applies."""
        a, b, _ = self._surface_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        return self.surface_samples(uniforms, a, b, surface, count_only=True, max_candidates=0)[2]

    def surface_region(self, uniforms, region, surface, other=None, max_level=None, select="cut", footprint=None, lasso=None, invert=False,
                       other_max_level=None, other_select="cut"):
        """Normal, variation and colour of each sample of a selection of THIS octree from its neighbours within surface.radius:
        A = query_region(region, max_level, select, footprint / lasso / invert); the neighbours come from A itself (other None) or from
        other.export_octree(other_max_level, other_select), a DeviceOctree on this device.  A count-only simlod_surface_samples call, the
        budget check, then the call with results -> an octree_io.SurfaceResult.  The budget is surface.max_candidates (None: 64 candidates
        per sample of A; 0: none); a count above it raises SimlodError naming numCandidates and maxCellPopulation — pick a smaller radius.
        With max_level=20, select="all" the colours are in the order paint_region's ARRAY paint takes: SurfaceResult.paint(dev, uniforms)
        writes them into the octree."""
        from .octree_io import SurfaceResult
        a, b, sel = self._surface_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        budget = self.COMPARE_BUDGET_PER_SAMPLE * a.num_samples if surface.max_candidates is None else surface.max_candidates
        c = self.surface_samples(uniforms, a, b, surface, count_only=True, max_candidates=0)[2]
        if budget != 0 and int(c["numCandidates"]) > budget:
            raise SimlodError(f"the surface of {a.num_samples} samples from {b.num_samples} at radius {float(surface.radius)} would test numCandidates = "
                              f"{int(c['numCandidates'])} pairs, above the budget of {budget} (maxCellPopulation = {int(c['maxCellPopulation'])} in "
                              f"{int(c['numCells'])} cells): pick a smaller radius or a coarser cut")
        records, colors, s = self.surface_samples(uniforms, a, b, surface, max_candidates=budget)
        if int(s["error"]) != 0:
            raise SimlodError(f"simlod_surface_samples reported error bits {int(s['error']):#x}; no record was written")
        return SurfaceResult(a, b, records, colors, s, surface, sel)

    # -- cluster queries (include/simlod_hip.h, "cluster queries") -------------------------------------------------------------------------
    def cluster_samples(self, uniforms, a, cluster, count_only=False, max_candidates=None):
        """One simlod_cluster_samples call on a sample array (as compare_samples takes them): per sample its connected component within
        cluster.radius.  -> (records: a uint8 tensor of abi.cluster_record_dtype records, colors: an int32 tensor of colour words, both on
        this device and in a's order, and the abi.cluster_summary_dtype record on the host); count_only: (None, None, record).  The call
        ALWAYS carries a candidate budget, compare_samples' (rule C6): max_candidates if given, else cluster.max_candidates, else 64
        candidates per sample; an explicit 0 is the opt-out.  A budget exceeded comes back as (None, None, record) with
        SIMLOD_CLUSTER_ERR_BUDGET in the record's error field."""
        u, up = self._u(uniforms)
        ta = self._samples_tensor(a)
        na = ta.numel() // abi.point_dtype.itemsize
        budget = max_candidates if max_candidates is not None else cluster.max_candidates
        pr = cluster.record(self.COMPARE_BUDGET_PER_SAMPLE * na if budget is None else int(budget))
        need = int(self.L.simlod_cluster_buffer_min_bytes(na))
        if need == 0:
            raise ValueError("numA is 1 .. 2^32 - 2")
        scratch = self._export_scratch(need)
        out = torch.zeros(abi.cluster_summary_dtype.itemsize, dtype=torch.uint8, device=self.device)
        records = colors = None
        if not count_only:
            records = torch.empty(na * abi.cluster_record_dtype.itemsize, dtype=torch.uint8, device=self.device)
            colors = torch.empty(na, dtype=torch.int32, device=self.device)
        opt = lambda t: None if t is None else self._p(t)
        _check(self.L.simlod_cluster_samples(up, self._p(ta), ctypes.c_uint64(na), ctypes.c_void_p(pr.ctypes.data), self._p(scratch),
                                             ctypes.c_uint64(scratch.numel()), opt(records), opt(colors), self._p(out), self._stream()),
               "simlod_cluster_samples")
        rec = out.cpu().numpy().view(abi.cluster_summary_dtype)[0]
        return (None, None, rec) if int(rec["error"]) != 0 else (records, colors, rec)

    def count_cluster(self, uniforms, region, cluster, max_level=None, select="cut", footprint=None, lasso=None, invert=False):
        """What cluster_region would cost: the abi.cluster_summary_dtype record of the count-only call (numCells, maxCellPopulation,
        numCandidates, the invalid count) for the same arguments; nothing is clustered and no budget applies."""
        a, _, _ = self._surface_inputs(uniforms, None, region, max_level, select, footprint, lasso, invert, None, "cut")
        return self.cluster_samples(uniforms, a, cluster, count_only=True, max_candidates=0)[2]

    def cluster_region(self, uniforms, region, cluster, max_level=None, select="cut", footprint=None, lasso=None, invert=False):
        """The clusters of a selection of THIS octree: A = query_region(region, max_level, select, footprint / lasso / invert), a count-only
        simlod_cluster_samples call, the budget check, then the call with results -> an octree_io.ClusterResult.  The budget is
        cluster.max_candidates (None: 64 candidates per sample of A; 0: none); a count above it raises SimlodError naming numCandidates and
        maxCellPopulation — pick a smaller radius or a coarser cut.  With max_level=20, select="all" the colours are in the order
        paint_region's ARRAY paint takes: ClusterResult.paint(dev, uniforms) writes them into the octree."""
        from .octree_io import ClusterResult
        a, _, sel = self._surface_inputs(uniforms, None, region, max_level, select, footprint, lasso, invert, None, "cut")
        budget = self.COMPARE_BUDGET_PER_SAMPLE * a.num_samples if cluster.max_candidates is None else cluster.max_candidates
        c = self.cluster_samples(uniforms, a, cluster, count_only=True, max_candidates=0)[2]
        if budget != 0 and int(c["numCandidates"]) > budget:
            raise SimlodError(f"clustering {a.num_samples} samples at radius {float(cluster.radius)} would test numCandidates = "
                              f"{int(c['numCandidates'])} pairs, above the budget of {budget} (maxCellPopulation = {int(c['maxCellPopulation'])} in "
                              f"{int(c['numCells'])} cells): pick a smaller radius or a coarser cut")
        records, colors, s = self.cluster_samples(uniforms, a, cluster, max_candidates=budget)
        if int(s["error"]) != 0:
            raise SimlodError(f"simlod_cluster_samples reported error bits {int(s['error']):#x}; no record is valid")
        return ClusterResult(a, records, colors, s, cluster, sel)

    # -- align queries (include/simlod_hip.h, "align queries") -----------------------------------------------------------------------------
    def align_scratch(self, a, b):
        """A scratch buffer of its own for align calls on `a` and `b` (sample arrays as compare_samples takes them, or their counts): the
        one a build call stamps and later reuse calls must be given unchanged (rule A7)."""
        na, nb = (v if isinstance(v, int) else self._samples_tensor(v).numel() // abi.point_dtype.itemsize for v in (a, b))
        need = int(self.L.simlod_align_buffer_min_bytes(na, nb))
        if need == 0:
            raise ValueError("numA and numB are 1 .. 2^32 - 2")
        return torch.empty(need, dtype=torch.uint8, device=self.device)

    def align_samples(self, uniforms, a, b, align, pose, scratch=None, reuse=False, records=False, count_only=False, max_candidates=None):
        """One simlod_align_samples call on two sample arrays (as compare_samples takes them; pass the SAME device tensor for `b` to every
        call that shares a grid): the samples of `a` moved by `pose` (3x4; None: the identity) against their nearest samples of `b` within
        align.radius.  -> (records: a uint8 tensor of abi.compare_record_dtype records on this device, or None unless records=True, and the
        abi.align_summary_dtype record on the host).  scratch: a buffer of align_scratch(a, b) (None: the octree's shared one, which the
        next query overwrites); reuse=True: the grid an earlier call built in `scratch` is reused (rule A7) — a grid that does not serve
        comes back as SIMLOD_ALIGN_ERR_GRID in the record's error field.  count_only: the grid's fields only.  The call ALWAYS carries a
        candidate budget, compare_samples' (rule C6): max_candidates if given, else align.max_candidates, else 64 candidates per sample of
        `a`; an explicit 0 is the opt-out.  With an error bit set no record was written: (None, record)."""
        u, up = self._u(uniforms)
        ta, tb = self._samples_tensor(a), self._samples_tensor(b)
        na, nb = ta.numel() // abi.point_dtype.itemsize, tb.numel() // abi.point_dtype.itemsize
        budget = max_candidates if max_candidates is not None else align.max_candidates
        flags = (abi.ALIGN_COUNT_ONLY if count_only else 0) | (abi.ALIGN_REUSE_GRID if reuse else 0)
        pr = align.record(pose, flags, self.COMPARE_BUDGET_PER_SAMPLE * na if budget is None else int(budget))
        need = int(self.L.simlod_align_buffer_min_bytes(na, nb))
        if need == 0:
            raise ValueError("numA and numB are 1 .. 2^32 - 2")
        if scratch is None:
            if reuse:
                raise ValueError("a reuse call needs the scratch buffer of the call that built the grid")
            scratch = self._export_scratch(need)
        out = torch.zeros(abi.align_summary_dtype.itemsize, dtype=torch.uint8, device=self.device)
        rec_t = torch.empty(na * abi.compare_record_dtype.itemsize, dtype=torch.uint8, device=self.device) if records and not count_only else None
        _check(self.L.simlod_align_samples(up, self._p(ta), ctypes.c_uint64(na), self._p(tb), ctypes.c_uint64(nb), ctypes.c_void_p(pr.ctypes.data),
                                           self._p(scratch), ctypes.c_uint64(scratch.numel()), None if rec_t is None else self._p(rec_t), self._p(out),
                                           self._stream()), "simlod_align_samples")
        rec = out.cpu().numpy().view(abi.align_summary_dtype)[0]
        return (None, rec) if int(rec["error"]) != 0 else (rec_t, rec)

    def register_samples(self, uniforms, a, b, align, pose=None, iterations=30, tol=None):
        """The registration of `a` onto `b` by ICP -> an octree_io.AlignResult: one scratch buffer (the octree's shared one, every
        query's: a first call pays for its allocation, which for gigabytes costs more than the steps), the first simlod_align_samples call builds the grid over `b` and every
        later one reuses it; each step reads its summary (one synchronisation), solves for the update on
        the host (octree_io.align_solve) and composes it into the pose.  It stops when the update moves no corner of A's bounding box by
        more than tol (None: size * 2^-22) or after `iterations` steps.  No record is written.  A step that reports an error bit raises
        SimlodError naming it."""
        from .octree_io import register_steps, _box_of
        u, _ = self._u(uniforms)
        ta, tb = self._samples_tensor(a), self._samples_tensor(b)
        mn, size = _box_of(u["boxMin"][0], u["boxMax"][0])
        xyz = ta.view(torch.float32).reshape(-1, 4)[:, :3]
        ok = torch.isfinite(xyz).all(dim=1, keepdim=True)
        inf = torch.tensor(float("inf"), device=self.device)
        lo, hi = torch.where(ok, xyz, inf).amin(dim=0).cpu().numpy().astype(np.float64), torch.where(ok, xyz, -inf).amax(dim=0).cpu().numpy().astype(np.float64)
        corners = np.array([[(lo, hi)[i >> k & 1][k] for k in range(3)] for i in range(8)]) if np.isfinite(lo).all() else np.zeros((0, 3))
        need = int(self.L.simlod_align_buffer_min_bytes(ta.numel() // abi.point_dtype.itemsize, tb.numel() // abi.point_dtype.itemsize))
        if need == 0:
            raise ValueError("numA and numB are 1 .. 2^32 - 2")
        scratch = self._export_scratch(need)                                    # (no other query runs on this octree between the steps)
        step = lambda T, first: self.align_samples(uniforms, ta, tb, align, T, scratch=scratch, reuse=not first)[1]
        res = register_steps(step, mn, size, corners, pose, iterations, tol)
        err = int(res.summaries[-1]["error"]) if res.summaries else 0
        if err != 0:
            s = res.summaries[-1]
            raise SimlodError(f"simlod_align_samples reported error bits {err:#x} at step {res.steps} (numCandidates = {int(s['numCandidates'])}, "
                              f"maxCellPopulation = {int(s['maxCellPopulation'])}): pick a smaller radius or a coarser cut of the other cloud")
        return res

    def count_align(self, uniforms, other, region, align, pose=None, max_level=None, select="cut", footprint=None, lasso=None, invert=False,
                    other_max_level=None, other_select="cut"):
        """What a step of register_region would cost: the abi.align_summary_dtype record of the count-only call (numCells, maxCellPopulation,
        numCandidates, the invalid counts) for the same arguments under `pose`; nothing is tested and no budget applies."""
        a, b, _ = self._compare_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        return self.align_samples(uniforms, a, b, align, pose, count_only=True, max_candidates=0)[1]

    def register_region(self, uniforms, other, region, align, pose=None, iterations=30, tol=None, max_level=None, select="cut", footprint=None,
                        lasso=None, invert=False, other_max_level=None, other_select="cut"):
        """The registration of a selection of THIS octree onto `other` (a DeviceOctree on this device): A = query_region(region, max_level,
        select, footprint / lasso / invert), B = other.export_octree(other_max_level, other_select), as compare_region selects them, then
        register_samples -> its octree_io.AlignResult with `a`, `b` and `selection` filled in.  AlignResult.transform(result.a.samples_tensor)
        gives the moved samples; neither octree is changed."""
        a, b, sel = self._compare_inputs(uniforms, other, region, max_level, select, footprint, lasso, invert, other_max_level, other_select)
        res = self.register_samples(uniforms, a, b, align, pose, iterations, tol)
        res.a, res.b, res.selection = a, b, sel
        return res

    # -- profile queries (include/simlod_hip.h, "profile queries") -------------------------------------------------------------------------
    def _profile(self, uniforms, profile, region, ml, sel, table, samples, records, sample_capacity, bound):
        """One simlod_query_profile call -> the SimlodQueryCounts record (host).  samples None: count only."""
        from .octree_io import Region
        u, up = self._u(uniforms)
        r, f = (Region() if region is None else region).record(), profile.record()
        nn = table.numel() // abi.export_node_dtype.itemsize
        counts = torch.zeros(abi.query_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        scratch = self._export_scratch(int(self.L.simlod_profile_buffer_min_bytes(nn, bound)))
        _check(self.L.simlod_query_profile(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(f.ctypes.data), ml, sel,
                                           self._p(scratch), ctypes.c_uint64(scratch.numel()), self._p(table), nn, None if samples is None else self._p(samples),
                                           ctypes.c_uint64(sample_capacity), None if records is None else self._p(records), self._p(counts), self._stream()),
               "simlod_query_profile")
        c = counts.cpu().numpy().view(abi.query_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"simlod_query_profile reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples)")
        return c

    def count_profile(self, uniforms, profile, region=None, max_level=None, select="cut"):
        """How much of the octree lies in the corridor of `profile` (an octree_io.Profile) and in `region` at `max_level`: the SimlodQueryCounts
        record of a count-only simlod_query_profile call.  No sample is written."""
        sel, ml, nn, bound = self._query_setup(max_level, select)
        return self._profile(uniforms, profile, region, ml, sel, self._table(nn), None, None, 0, bound)

    def query_profile(self, uniforms, profile, region=None, max_level=None, select="cut", return_counts=False):
        """The samples in the corridor of `profile` (an octree_io.Profile) — and in `region`, an octree_io.Region — as an octree_io.OctreeExport on
        this device (select abi.EXPORT_REGION), and their records: a uint8 tensor of numSamples x abi.profile_sample_dtype (station along the
        polyline, signed offset from the segment's line, height, segment), records[k] for samples[k].  A count-only call first, then the
        outputs sized exactly.  Raises SimlodError when the device reports an error."""
        from .octree_io import OctreeExport
        sel, ml, nn, bound = self._query_setup(max_level, select)
        c = self._profile(uniforms, profile, region, ml, sel, self._table(nn), None, None, 0, bound)
        nn, ns = int(c["numNodes"]), int(c["numSamples"])
        table = torch.empty(nn * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)
        samples = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        records = torch.empty(max(ns, 1) * abi.profile_sample_dtype.itemsize, dtype=torch.uint8, device=self.device)
        c = self._profile(uniforms, profile, region, ml, sel, table, samples, records, ns, bound)
        u = np.asarray(uniforms).reshape(-1)[0]
        ns = int(c["numSamples"])
        ex = OctreeExport(table, samples[: ns * abi.point_dtype.itemsize], u["boxMin"], u["boxMax"], ml, abi.EXPORT_REGION)
        records = records[: ns * abi.profile_sample_dtype.itemsize]
        return (ex, records, c) if return_counts else (ex, records)

    # -- view queries (include/simlod_hip.h, "view queries") -------------------------------------------------------------------------------
    def _view(self, uniforms, view, ml, table, samples, sample_capacity, bound):
        """One simlod_query_view call -> the SimlodViewCounts record (host).  samples None: count only.  SIMLOD_EXPORT_ERR_BUDGET is the
        caller's to judge; any other error bit raises SimlodError."""
        u, up = self._u(uniforms)
        nn = table.numel() // abi.export_node_dtype.itemsize
        counts = torch.zeros(abi.view_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        scratch = self._export_scratch(int(self.L.simlod_export_buffer_min_bytes(nn, bound)))
        _check(self.L.simlod_query_view(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(view.ctypes.data), ml, self._p(scratch),
                                        ctypes.c_uint64(scratch.numel()), self._p(table), nn, None if samples is None else self._p(samples),
                                        ctypes.c_uint64(sample_capacity), self._p(counts), self._stream()), "simlod_query_view")
        c = counts.cpu().numpy().view(abi.view_counts_dtype)[0]
        if int(c["error"]) & ~abi.EXPORT_ERR_BUDGET:
            raise SimlodError(f"simlod_query_view reported error bits {int(c['error']):#x} (counts: {int(c['numNodes'])} nodes, {int(c['numSamples'])} samples)")
        return c

    def count_view(self, uniforms, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None):
        """What the camera of `uniforms` (width, height, transform_updateBound, minNodeSize, the box) would take from the octree: the
        SimlodViewCounts record of a count-only simlod_query_view call — the chosen bias (the smallest in [bias, max_bias] whose cut holds at
        most `budget` samples; error has abi.EXPORT_ERR_BUDGET when none does), numSamples, numSelected, numInside and the ladder samplesAt[b]
        of every bias.  No frame is rendered, nothing is copied, the octree's frame state stays as it is."""
        _, ml, nn, _ = self._query_setup(max_level, "all")
        return self._view(uniforms, abi.view_record(bias, max_bias, budget, cull, draw_small_root), ml, self._table(nn), None, 0, 0)

    def query_view(self, uniforms, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None, return_counts=False):
        """The cut the camera of `uniforms` needs as an octree_io.OctreeExport on this device (select abi.EXPORT_VISIBLE): what render(uniforms
        with minNodeSize * 2^bias) followed by export_octree(select="visible") gives, without the frame.  A count-only call first, then the
        outputs sized exactly.  When no bias in [bias, max_bias] fits `budget`: SimlodError — or, return_counts, the table of max_bias without
        samples and counts whose error has abi.EXPORT_ERR_BUDGET."""
        from .octree_io import OctreeExport
        _, ml, nn, _ = self._query_setup(max_level, "all")
        view = abi.view_record(bias, max_bias, budget, cull, draw_small_root)
        c = self._view(uniforms, view, ml, self._table(nn), None, 0, 0)
        if int(c["error"]) & abi.EXPORT_ERR_BUDGET and not return_counts:
            raise SimlodError(f"simlod_query_view: no bias in [{int(bias)}, {int(max_bias)}] fits {int(budget)} samples (the coarsest holds {int(c['numSamples'])})")
        nn, ns = int(c["numNodes"]), int(c["numSamples"])
        table = torch.empty(nn * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)
        samples = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        c = self._view(uniforms, view, ml, table, samples, ns, ns)
        written = 0 if int(c["error"]) & abi.EXPORT_ERR_BUDGET else int(c["numSamples"])
        u = np.asarray(uniforms).reshape(-1)[0]
        ex = OctreeExport(table, samples[: written * abi.point_dtype.itemsize], u["boxMin"], u["boxMax"], ml, abi.EXPORT_VISIBLE)
        return (ex, c) if return_counts else ex

    # -- view deltas (include/simlod_hip.h, "view deltas") -------------------------------------------------------------------------------
    def _held_table(self, held):
        """(the held table as a uint8 tensor on this device or None, its entries)"""
        if held is None or held.num_nodes == 0:
            return None, 0
        return held.table_tensor.to(self.device), held.num_nodes

    def _view_delta(self, uniforms, view, ml, held_t, num_held, tails, table, entries, delta, delta_capacity, dropped, dropped_capacity, bound):
        """One simlod_query_view_delta call -> the SimlodDeltaCounts record (host).  delta None: count only; dropped None: counted only.
        SIMLOD_EXPORT_ERR_BUDGET is the caller's to judge; any other error bit raises SimlodError."""
        u, up = self._u(uniforms)
        nn = table.numel() // abi.export_node_dtype.itemsize
        counts = torch.zeros(abi.delta_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        scratch = self._export_scratch(int(self.L.simlod_view_delta_buffer_min_bytes(nn, bound, num_held)))
        opt = lambda t: None if t is None else self._p(t)
        _check(self.L.simlod_query_view_delta(self._p(self.nodes), self._p(self.stats), up, ctypes.c_void_p(view.ctypes.data), ml, opt(held_t), num_held,
                                              abi.DELTA_TAILS if tails else 0, self._p(scratch), ctypes.c_uint64(scratch.numel()), self._p(table), nn,
                                              self._p(entries), opt(delta), ctypes.c_uint64(delta_capacity), opt(dropped), dropped_capacity, self._p(counts),
                                              self._stream()), "simlod_query_view_delta")
        c = counts.cpu().numpy().view(abi.delta_counts_dtype)[0]
        if int(c["view"]["error"]) & ~abi.EXPORT_ERR_BUDGET:
            raise SimlodError(f"simlod_query_view_delta reported error bits {int(c['view']['error']):#x} ({int(c['view']['numNodes'])} nodes, {int(c['numDeltaSamples'])} delta samples)")
        return c

    def _entries(self, nn):
        return torch.empty(max(nn, 1) * abi.delta_entry_dtype.itemsize, dtype=torch.uint8, device=self.device)

    def count_view_delta(self, uniforms, held, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None, tails=False):
        """What the camera of `uniforms` needs on top of the cut `held` (an octree_io.OctreeExport, or None): the SimlodDeltaCounts record of a
        count-only simlod_query_view_delta call — the view's counts as count_view gives them, numDeltaSamples, numKeptSamples, the entries kept,
        grown and added, and the held entries to drop.  No sample is written."""
        _, ml, nn, _ = self._query_setup(max_level, "all")
        held_t, nh = self._held_table(held)
        return self._view_delta(uniforms, abi.view_record(bias, max_bias, budget, cull, draw_small_root), ml, held_t, nh, tails, self._table(nn),
                                self._entries(nn), None, 0, None, 0, 0)

    def query_view_delta(self, uniforms, held, bias=0, max_bias=abi.VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False, max_level=None,
                         tails=False, return_counts=False):
        """The cut the camera of `uniforms` needs, as a difference to the cut `held` (an octree_io.OctreeExport — a table this library wrote —
        or None): an octree_io.ViewDelta on this device with the new cut's table, per entry what the receiver holds of it (KEPT, GROWN under
        tails=True, else ADDED), the samples it lacks, and the held entries to drop.  A count-only call first, then the outputs sized exactly.
        tails=True sends only the new samples of a node that grew: not across a reset, an import or a colour-filter launch.  When no bias in
        [bias, max_bias] fits `budget`: SimlodError — or, return_counts, an empty delta whose counts["view"]["error"] has abi.EXPORT_ERR_BUDGET."""
        from .octree_io import ViewDelta
        _, ml, nn, _ = self._query_setup(max_level, "all")
        view = abi.view_record(bias, max_bias, budget, cull, draw_small_root)
        held_t, nh = self._held_table(held)
        c = self._view_delta(uniforms, view, ml, held_t, nh, tails, self._table(nn), self._entries(nn), None, 0, None, 0, 0)
        if int(c["view"]["error"]) & abi.EXPORT_ERR_BUDGET and not return_counts:
            raise SimlodError(f"simlod_query_view_delta: no bias in [{int(bias)}, {int(max_bias)}] fits {int(budget)} samples (the coarsest holds {int(c['view']['numSamples'])})")
        nn, ns, nd = int(c["view"]["numNodes"]), int(c["numDeltaSamples"]), int(c["numDropped"])
        table = torch.empty(nn * abi.export_node_dtype.itemsize, dtype=torch.uint8, device=self.device)
        entries = torch.empty(nn * abi.delta_entry_dtype.itemsize, dtype=torch.uint8, device=self.device)
        delta = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        dropped = torch.empty(max(nd, 1) * 4, dtype=torch.uint8, device=self.device)
        c = self._view_delta(uniforms, view, ml, held_t, nh, tails, table, entries, delta, ns, dropped, nd, ns)
        u = np.asarray(uniforms).reshape(-1)[0]
        vd = ViewDelta(table, entries, delta[: int(c["numDeltaSamples"]) * abi.point_dtype.itemsize], dropped[: int(c["numDropped"]) * 4], u["boxMin"], u["boxMax"], ml, c)
        return (vd, c) if return_counts else vd

    def merge_view_delta(self, held, delta):
        """The new cut as an octree_io.OctreeExport on this device (select abi.EXPORT_VISIBLE) from the cut `held` (the OctreeExport the delta
        was taken against, or None) and `delta` (an octree_io.ViewDelta): one simlod_merge_view_delta call."""
        from .octree_io import OctreeExport
        held_t, nh = self._held_table(held)
        held_s = None if held_t is None else held.samples_tensor.to(self.device)
        table, entries, dl = (t.to(self.device) for t in (delta.table_tensor, delta.entries_tensor, delta.samples_tensor))
        nn = delta.num_nodes
        ns = int(delta.counts["numDeltaSamples"]) + int(delta.counts["numKeptSamples"])
        scratch = self._export_scratch(int(self.L.simlod_view_delta_buffer_min_bytes(nn, ns, nh)))
        samples = torch.empty(max(ns, 1) * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
        counts = torch.zeros(abi.export_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        opt = lambda t: None if t is None or t.numel() == 0 else self._p(t)
        _check(self.L.simlod_merge_view_delta(opt(held_t), nh, opt(held_s), self._p(table), self._p(entries), nn, opt(dl), self._p(scratch),
                                              ctypes.c_uint64(scratch.numel()), self._p(samples), ctypes.c_uint64(ns), self._p(counts), self._stream()),
               "simlod_merge_view_delta")
        c = counts.cpu().numpy().view(abi.export_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"simlod_merge_view_delta reported error bits {int(c['error']):#x} ({int(c['numNodes'])} nodes, {int(c['numSamples'])} samples)")
        return OctreeExport(table, samples[: int(c["numSamples"]) * abi.point_dtype.itemsize], delta.box_min, delta.box_max, delta.max_level, abi.EXPORT_VISIBLE)

    # -- packed samples (include/simlod_hip.h, "packed samples") ---------------------------------------------------------------------------
    def _pack_call(self, unpack, obj, src, dst, entries):
        """One simlod_pack_samples / simlod_unpack_samples call on the arrays of `obj` -> the SimlodPackCounts record (host); error bits raise."""
        name = "simlod_unpack_samples" if unpack else "simlod_pack_samples"
        if obj.num_nodes == 0:
            raise SimlodError(f"{name}: an empty table")
        u = np.zeros(1, dtype=abi.uniforms_dtype)
        u["boxMin"], u["boxMax"] = obj.box_min, obj.box_max
        table = obj.table_tensor.to(self.device)
        n = src.numel() // (8 if unpack else abi.point_dtype.itemsize)
        scratch = self._export_scratch(int(self.L.simlod_pack_buffer_min_bytes(obj.num_nodes, n)))
        counts = torch.zeros(abi.pack_counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        call = self.L.simlod_unpack_samples if unpack else self.L.simlod_pack_samples
        _check(call(ctypes.c_void_p(u.ctypes.data), self._p(table), None if entries is None else self._p(entries), obj.num_nodes, self._p(src),
                    ctypes.c_uint64(n), self._p(scratch), ctypes.c_uint64(scratch.numel()), self._p(dst), self._p(counts), self._stream()), name)
        c = counts.cpu().numpy().view(abi.pack_counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"{name} reported error bits {int(c['error']):#x} ({int(c['numSamples'])} of {n} samples)")
        return table, c

    def pack(self, obj, return_counts=False):
        """`obj` (an octree_io.OctreeExport or ViewDelta, on any device) with 8-byte samples: a PackedExport / PackedViewDelta on this device —
        one simlod_pack_samples call.  return_counts: also the SimlodPackCounts record (numClamped, numInexact, numAlpha)."""
        from .octree_io import PackedExport, PackedViewDelta, ViewDelta
        delta = isinstance(obj, ViewDelta)
        src = obj.samples_tensor.to(self.device)
        entries = obj.entries_tensor.to(self.device) if delta else None
        n = obj.num_samples
        if n == 0:                                                              # (no array to give the call)
            packed, c, table = torch.zeros(0, dtype=torch.uint8, device=self.device), np.zeros((), dtype=abi.pack_counts_dtype), obj.table_tensor.to(self.device)
        else:
            packed = torch.zeros(n * 8, dtype=torch.uint8, device=self.device)
            table, c = self._pack_call(False, obj, src, packed, entries)
        if delta:
            out = PackedViewDelta(table, entries, packed, obj.dropped_tensor.to(self.device), obj.box_min, obj.box_max, obj.max_level, obj.counts)
        else:
            out = PackedExport(table, packed, obj.box_min, obj.box_max, obj.max_level, obj.select)
        return (out, c) if return_counts else out

    def unpack(self, obj, return_counts=False):
        """`obj` (an octree_io.PackedExport or PackedViewDelta) with 16-byte samples again: an OctreeExport / ViewDelta on this device — one
        simlod_unpack_samples call."""
        from .octree_io import OctreeExport, PackedViewDelta, ViewDelta
        delta = isinstance(obj, PackedViewDelta)
        src = obj.packed_tensor.to(self.device)
        entries = obj.entries_tensor.to(self.device) if delta else None
        n = obj.num_samples
        if n == 0:
            samples, c, table = torch.zeros(0, dtype=torch.uint8, device=self.device), np.zeros((), dtype=abi.pack_counts_dtype), obj.table_tensor.to(self.device)
        else:
            samples = torch.zeros(n * abi.point_dtype.itemsize, dtype=torch.uint8, device=self.device)
            table, c = self._pack_call(True, obj, src, samples, entries)
        if delta:
            out = ViewDelta(table, entries, samples, obj.dropped_tensor.to(self.device), obj.box_min, obj.box_max, obj.max_level, obj.counts)
        else:
            out = OctreeExport(table, samples, obj.box_min, obj.box_max, obj.max_level, obj.select)
        return (out, c) if return_counts else out

    # -- pair queries: what the ray and the neighbour query share (csrc/export_pairs.inc) ------------------------------------------------------
    # per C call simlod_query_<what>: the record's dtype, its name in messages, its C name, the counts record's dtype.  What _pair_query
    # relies on (include/simlod_hip.h), with `ks` the query's own scalars and `outs` its result pointers, each in the header's order:
    #   simlod_<what>_buffer_min_bytes(nodeCapacity, sampleBound, numRecords, *ks, numPairs, numCandidates)
    #   simlod_query_<what>(nodes, stats, uniforms, records, numRecords, *ks, maxLevel, select, scratch, scratchBytes, table, tableCapacity,
    #                       *outs, counts, stream)
    #   rays: ks = (), outs = (hits,);  neighbours: ks = (k,), outs = (neighbours, within)
    _PAIR_QUERIES = {"rays": (abi.ray_dtype, "rays", "SimlodRay", abi.ray_counts_dtype),
                     "neighbours": (abi.sphere_dtype, "spheres", "SimlodSphere", abi.neighbour_counts_dtype)}

    def _pair_query(self, what, uniforms, records, ks, max_level, select, outs, counts_of=None):
        """One simlod_query_<what> call -> its counts record (host).  `records`: a uint8 device tensor of the query's records; ks: the arguments
        behind the record count ((k,) for neighbours); outs: the result tensors, None each in a count-only call; counts_of: the counts of a
        count-only call, from which a call with results sizes its scratch."""
        rec_dtype, _, _, counts_dtype = self._PAIR_QUERIES[what]
        u, up = self._u(uniforms)
        sel, ml, nn, bound = self._query_setup(max_level, select)
        n = records.numel() // rec_dtype.itemsize
        pairs, candidates = (0, 0) if counts_of is None else (int(counts_of["numPairs"]), int(counts_of["numCandidates"]))
        scratch = self._export_scratch(int(getattr(self.L, f"simlod_{what}_buffer_min_bytes")(nn, bound, n, *ks, pairs, candidates)))
        counts = torch.zeros(counts_dtype.itemsize, dtype=torch.uint8, device=self.device)
        fn = f"simlod_query_{what}"
        _check(getattr(self.L, fn)(self._p(self.nodes), self._p(self.stats), up, self._p(records), n, *ks, ml, sel, self._p(scratch),
                                   ctypes.c_uint64(scratch.numel()), None, nn, *(None if o is None else self._p(o) for o in outs), self._p(counts),
                                   self._stream()), fn)
        c = counts.cpu().numpy().view(counts_dtype)[0]
        if int(c["error"]) != 0:
            raise SimlodError(f"{fn} reported error bits {int(c['error']):#x} ({int(c['numNodes'])} nodes, {int(c['numPairs'])} pairs)")
        return c

    def _records_tensor(self, what, records):
        """The records of a simlod_query_<what> call (an octree_io.Rays / Spheres, or a device tensor of whole records) as a uint8 tensor on
        this octree's device."""
        dtype, name, struct, _ = self._PAIR_QUERIES[what]
        if isinstance(records, torch.Tensor):
            t = records.reshape(-1).view(torch.uint8)
            if t.device != self.device or t.numel() == 0 or t.numel() % dtype.itemsize:
                raise SimlodError(f"{name}: a non-empty tensor of whole {struct} records on this octree's device")
            return t
        rec = np.ascontiguousarray(records.record())
        if len(rec) == 0:
            raise SimlodError(f"{name}: an empty batch")
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(self.device)

    # -- ray queries (include/simlod_hip.h, "ray queries") ---------------------------------------------------------------------------------
    def count_rays(self, uniforms, rays, max_level=None, select="cut"):
        """The SimlodRayCounts record of a count-only simlod_query_rays call (numNodes, numHits, numInvalid, numPairs, numCandidates)."""
        return self._pair_query("rays", uniforms, self._records_tensor("rays", rays), (), max_level, select, (None,))

    def cast_rays(self, uniforms, rays, max_level=None, select="cut", return_counts=False):
        """The first sample in the cone along each ray (an octree_io.Rays, or a device tensor of SimlodRay records): a count-only call, scratch
        sized from its counts, then the hits — a numpy record array (abi.ray_hit_dtype) for host rays, a uint8 device tensor of the same
        records for device rays.  `node` / `ordinal` refer to export_octree(max_level, select).  A miss has t = inf and node = EXPORT_NONE."""
        t = self._records_tensor("rays", rays)
        c = self._pair_query("rays", uniforms, t, (), max_level, select, (None,))
        hits = torch.empty(t.numel() // abi.ray_dtype.itemsize * abi.ray_hit_dtype.itemsize, dtype=torch.uint8, device=self.device)
        c = self._pair_query("rays", uniforms, t, (), max_level, select, (hits,), c)
        out = hits if isinstance(rays, torch.Tensor) else hits.cpu().numpy().view(abi.ray_hit_dtype)
        return (out, c) if return_counts else out

    # -- neighbour queries (include/simlod_hip.h, "neighbour queries") ---------------------------------------------------------------------
    @staticmethod
    def _k(k):
        if not 1 <= int(k) <= abi.NEIGHBOURS_MAX_K:
            raise SimlodError(f"k = {k}: 1 .. {abi.NEIGHBOURS_MAX_K}")
        return int(k)

    def count_neighbours(self, uniforms, spheres, k, max_level=None, select="cut"):
        """The SimlodNeighbourCounts record of a count-only simlod_query_neighbours call (numNodes, numInvalid, numPairs, numCandidates;
        numFound and numWithin are 0: no sample is tested)."""
        k = self._k(k)
        return self._pair_query("neighbours", uniforms, self._records_tensor("neighbours", spheres), (k,), max_level, select, (None, None))

    def find_neighbours(self, uniforms, spheres, k, max_level=None, select="cut", return_counts=False):
        """The k nearest samples within the radius of each query (an octree_io.Spheres, or a device tensor of SimlodSphere records): a
        count-only call, scratch sized from its counts, then the results -> (neighbours, within).  Host queries: an (n, k) numpy record array
        (abi.neighbour_dtype) and an int array; device queries: a uint8 device tensor of the same records and a device tensor of n int32
        counts.  `node` / `ordinal` refer to export_octree(max_level, select).  The places behind min(k, within) hold d2 = inf and
        node = EXPORT_NONE."""
        k = self._k(k)
        t = self._records_tensor("neighbours", spheres)
        n = t.numel() // abi.sphere_dtype.itemsize
        c = self._pair_query("neighbours", uniforms, t, (k,), max_level, select, (None, None))
        out = torch.empty(n * k * abi.neighbour_dtype.itemsize, dtype=torch.uint8, device=self.device)
        within = torch.empty(n, dtype=torch.int32, device=self.device)
        c = self._pair_query("neighbours", uniforms, t, (k,), max_level, select, (out, within), c)
        if not isinstance(spheres, torch.Tensor):
            out, within = out.cpu().numpy().view(abi.neighbour_dtype).reshape(n, k), within.cpu().numpy().view(np.uint32).astype(np.int64)
        return (out, within, c) if return_counts else (out, within)

    def k_nearest(self, uniforms, points, k, radius0, max_level=None, select="cut"):
        """The k nearest samples of each position without a radius of the caller's: `points` are abi.point_dtype records or an (n, 3) array on
        the host.  Queries every position at radius0, then only the positions with within < k again at twice the radius, until every position
        has k or the radius exceeds the box diagonal -> (neighbours, within) as find_neighbours returns them for host queries.  A position
        with within >= k has its exact k nearest; one with fewer (the octree holds fewer than k samples within the last radius) has them all.
        Every doubling is a find_neighbours call of its own: two C calls and a device round trip for the counts and the results, so choose
        radius0 near the expected distance of the k-th neighbour."""
        from .octree_io import Spheres
        p = np.asarray(points)
        centers = np.stack([p["x"], p["y"], p["z"]], axis=1) if p.dtype.names else p.reshape(-1, 3)
        centers = centers.astype(np.float32)
        n, k = len(centers), int(k)
        u = np.asarray(uniforms).reshape(-1)[0]
        diag = float(np.sqrt(3.0) * (np.asarray(u["boxMax"], np.float32) - np.asarray(u["boxMin"], np.float32)).max())
        out = np.zeros((n, k), dtype=abi.neighbour_dtype)
        out["d2"], out["node"], out["ordinal"] = np.inf, abi.EXPORT_NONE, abi.EXPORT_NONE
        within = np.zeros(n, np.int64)
        todo, r = np.arange(n), np.float32(radius0)
        if not (np.isfinite(r) and r > 0):
            raise SimlodError("k_nearest: radius0 must be positive and finite")
        while len(todo):
            nb, w = self.find_neighbours(uniforms, Spheres(centers[todo], r), k, max_level, select)
            out[todo], within[todo] = nb, w
            todo = todo[w < k]
            if float(r) > diag:
                break
            r = np.float32(2.0) * r
        return out, within

    def import_octree(self, export, check=True, *, buildable=False, uniforms=None):
        """Replace this object's octree by `export` (an octree_io.OctreeExport on the host or on a device): simlod_import_octree validates the
        table on the device and writes a renderable octree into the node array and the persistent buffer.  check: read Stats back and raise
        SimlodError when the table failed validation (SIMLOD_ERR_IMPORT).  Until the next reset, construct() and colorfilter() refuse it.

        buildable=True: simlod_import_octree_buildable — the occupancy grids and a builder state as after a reset too, so that construct()
        goes on ingesting into the octree.  `uniforms` (required) give the box, which must be the export's, and the persistent capacity; the
        export must be a full one (select "all", max_level 20: OctreeExport.validate(buildable=True)).  Both are checked here, before anything
        is enqueued (SimlodError).  check=True also raises on SIMLOD_ERR_IMPORT_GRID (a grid disagrees with the table: the wrong box)."""
        if buildable:
            if uniforms is None:
                raise SimlodError("import_octree(buildable=True) needs the uniforms the octree goes on being built with")
            u0 = np.asarray(uniforms).reshape(-1)[0]
            if tuple(np.asarray(u0["boxMin"], np.float32).tolist()) != export.box_min or tuple(np.asarray(u0["boxMax"], np.float32).tolist()) != export.box_max:
                raise SimlodError(f"import_octree(buildable=True): the uniforms' box {tuple(u0['boxMin'])}..{tuple(u0['boxMax'])} is not the export's "
                                  f"{export.box_min}..{export.box_max}")
            try:
                export.validate(buildable=True)
            except ValueError as e:
                raise SimlodError(f"import_octree(buildable=True): {e}") from None
        table = export.table_tensor.to(self.device)
        samples = export.samples_tensor.to(self.device)
        n, m = export.num_nodes, export.num_samples
        need = int(self.L.simlod_export_buffer_min_bytes(n, m))
        scratch = self._export_scratch(need)
        if buildable:
            u, up = self._u(uniforms)
            _check(self.L.simlod_import_octree_buildable(up, self._p(table), n, self._p(samples), ctypes.c_uint64(m), self._p(scratch),
                                                         ctypes.c_uint64(scratch.numel()), self._p(self.persistent), self._p(self.nodes), self._p(self.stats),
                                                         self._p(self.num_uploaded), self._p(self.batch_sizes), self._stream()), "simlod_import_octree_buildable")
            what, bits = "simlod_import_octree_buildable", abi.SIMLOD_ERR_IMPORT | abi.SIMLOD_ERR_IMPORT_GRID
        else:
            _check(self.L.simlod_import_octree(self._p(table), n, self._p(samples), ctypes.c_uint64(m), self._p(scratch), ctypes.c_uint64(scratch.numel()),
                                               self._p(self.persistent), ctypes.c_uint64(self.persistent_bytes), self._p(self.nodes), self._p(self.stats),
                                               self._stream()), "simlod_import_octree")
            what, bits = "simlod_import_octree", abi.SIMLOD_ERR_IMPORT
        self.uploaded_host = self.processed_host = 0
        if check:
            dbg = int(self.read_stats()["dbg"]) & bits
            if dbg & abi.SIMLOD_ERR_IMPORT:
                raise SimlodError(f"{what}: the table failed validation on the device (SIMLOD_ERR_IMPORT)")
            if dbg & abi.SIMLOD_ERR_IMPORT_GRID:
                raise SimlodError(f"{what}: a rebuilt occupancy grid disagrees with the table — not the box the octree was built with (SIMLOD_ERR_IMPORT_GRID)")

    def download_image(self):
        """(nodes, persistent, numNodes, device base addresses) — the octree image as host arrays, pointers untouched."""
        torch.cuda.synchronize(self.device)
        stats = self.read_stats()
        used = int(stats["allocatedBytes_persistent"])
        if used == 0:   # before the first construct the stats pass has not run: read the allocator header
            used = int(self.persistent[8:16].cpu().numpy().view(np.uint64)[0])
        n = int(stats["numNodes"])
        nodes = self.nodes[: n * 152].cpu().numpy().view(abi.node_dtype).copy()
        pers = self.persistent[:used].cpu().numpy().copy()
        return nodes, pers, n, self.nodes.data_ptr(), self.persistent.data_ptr()
