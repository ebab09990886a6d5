"""GPU tier: a frame at 129 x 97 — 12 513 pixels, an odd count, so the 8-byte and the 4-byte planes each end in a partial 16-byte unit: the tail
branch of clear_frame and every rounding step of the frame layout (simlod_amd/csrc/render_layout.hpp), which no frame at a round size takes — and the
runtime's readers of the render buffer, which take every offset from DeviceOctree.frame_layout."""
import numpy as np
import pytest

import cases
from simlod_amd import abi
from test_gpu_parity import _device, _ingest
from util import assert_frame_equals_oracle, host_image_of, oracle_frame

pytestmark = pytest.mark.gpu
W, H = 129, 97
_BUILT = {}


def _octree():
    """(device, box, transform, host image) of the uniform_3x40k case, built once."""
    if not _BUILT:
        pts, box, batch, _ = cases.case("uniform_3x40k")
        dev = _device(persistent_bytes=1 << 30, ring_slots=4)
        T = cases.shifted_cam(box, (0.0, 0.0, 0.0), W, H)
        _ingest(dev, dev.uniforms(W, H, T, box), cases.batches_of("uniform_3x40k", pts, batch))
        assert int(dev.read_stats()["dbg"]) == 0
        _BUILT["octree"] = (dev, box, T) + host_image_of(dev)
    return _BUILT["octree"]


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
def test_frame_with_an_odd_pixel_count_and_the_layout_readers(built_libs, hqs):
    dev, box, T, nodes, pers, nn = _octree()
    u = dev.uniforms(W, H, T, box, hqs=hqs, min_node_size=16.0)      # (at this size the cube spans 50 pixels: with the default 64 nothing is large enough to be drawn)
    lay = dev.frame_layout(W, H)
    assert (W * H) % 2 == 1 and lay["colour"] - lay["depth"] > W * H * 4 and lay["work"] - lay["framebuffer"] > W * H * 8      # both planes end in a partial unit
    dev.render_buffer.fill_(0xA5)           # nothing a frame reads may be left over from the frame before
    dev.render(u)
    fb_dev, col_dev, st, vis = assert_frame_equals_oracle(dev, nodes, nn, u, f"129x97 hqs={hqs}", 1000)
    fb, col, _, _ = oracle_frame(nodes, nn, u)
    worst = int(np.abs(col_dev.view(np.uint8).astype(np.int16) - col.view(np.uint8).astype(np.int16)).max())
    print(f"129x97 hqs={hqs}: {int((fb != abi.CLEAR_PIXEL).sum())} pixels drawn, RGBA8 differs from the oracle's in {int((col_dev != col).sum())} pixels, by at most {worst}")
    assert np.array_equal(fb_dev, fb) and worst <= 1          # the pre-EDL frame bit for bit; RGBA8 within 1 per channel (log2 / exp come from two maths libraries)
    # the frame's own counter of visible nodes, read through the layout, is what r_output copied into Stats
    _, early = dev.visible_records_early()
    assert int(early.item()) == int(dev.read_stats()["numVisibleNodes"]) == int(st["numVisibleNodes"]) > 0
    # the same frame in four parts: the planes the composition reduces, where frame_layout says they are
    dev.render_buffer.fill_(0xA5)
    dev.render_composed(u)
    assert np.array_equal(dev.framebuffer(W, H), fb) and np.array_equal(dev.color(W, H), col_dev)
    base = dev.render_buffer.data_ptr()
    for plane, name, elems in ((dev.depth_plane(), "depth", W * H), (dev.sum_planes(), "sums", 4 * W * H), (dev.framebuffer_words(), "framebuffer", W * H)):
        assert plane.numel() == elems and plane.data_ptr() - base == lay[name], name
    assert np.array_equal(dev.framebuffer_words().cpu().numpy().view(np.uint64), fb)
    if hqs:
        d = dev.depth_plane().cpu().numpy().view(np.uint32)
        f = d.view(np.float32)
        assert ((d == 0x7F800000) | (np.isfinite(f) & (f > 0.0))).all(), "a depth word is neither the clear value nor a depth"
        assert d[-1] == 0x7F800000 or (fb[-1] >> np.uint64(32)) == d[-1]                   # the plane's last, odd element: cleared by the tail path (or drawn)
    visible_samples = int(st["numVisiblePoints"]) + int(st["numVisibleVoxels"])
    assert 0 <= dev.samples_binned(W, H) + dev.samples_outside_tiles() <= visible_samples
    assert dev.lists_read_through_table() <= int(st["numVisibleNodes"])
