"""Two octrees in ONE context (simlod_context_attach puts B's node array into A's), their launches interleaved around a
simlod_octree_image_replaced(A): what the library keeps per octree between launches — the leaf chunk table, the side tables' stale flag, the
launch feedback — must stay with its own node array.  Both octrees against the port oracle: Stats, the whole dump, and A's frame."""
import pytest

import oracle
from cases import H, W, batches_of, case
from test_gpu_parity import _device
from util import STATS_BUILD_FIELDS, assert_dumps_equal, assert_frame_equals_oracle, assert_stats_equal, host_image_of

pytestmark = pytest.mark.gpu

PERSISTENT = 1 << 30


def _oracle_after(u, pts, batch):
    ref = oracle.HostOctree("port", persistent_bytes=PERSISTENT, ring_slots=8)
    ref.reset(u)
    ref.add_points(u, pts, batch)
    assert ref.last_error() == 0
    return ref


def test_two_octrees_in_one_context_keep_their_own_state_across_an_image_replaced(built_libs):
    pa, box_a, batch_a, Ta = case("terrain_4x100k")
    pb, box_b, batch_b, Tb = case("uniform_3x40k")
    ba, bb = batches_of("terrain_4x100k", pa, batch_a), batches_of("uniform_3x40k", pb, batch_b)
    assert len(ba) == 4 and len(bb) == 3
    A = _device(persistent_bytes=PERSISTENT, ring_slots=8)
    B = _device(persistent_bytes=PERSISTENT, ring_slots=8)
    try:
        assert A.L.simlod_context_attach(A.ctx, B._p(B.nodes)) == 0      # both node arrays in A's context: B's launches run with A's knobs
        A.tune("SIMLOD_EXACT_GROUP", 1)
        ua, ub = A.uniforms(W, H, Ta, box_a), B.uniforms(W, H, Tb, box_b)

        def ingest(dev, u, batches, done):
            for k, b in enumerate(batches):
                dev.upload(b)
                dev.construct(u)
                assert dev.processed() == done + k + 1

        A.reset(ua)
        ingest(A, ua, ba[:2], 0)
        assert A.L.simlod_octree_image_replaced(A._p(A.nodes)) == 0
        B.reset(ub)
        ingest(B, ub, bb[:1], 0)
        ingest(A, ua, ba[2:], 2)
        ingest(B, ub, bb[1:], 1)
        A.render(ua)

        images = {}
        for name, dev, u, pts, batch in (("A", A, ua, pa, batch_a), ("B", B, ub, pb, batch_b)):
            ref = _oracle_after(u, pts, batch)
            ds = dev.read_stats()
            assert int(ds["dbg"]) == 0, f"{name}: Stats.dbg={int(ds['dbg']):#x}"
            assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, name)
            images[name] = nodes, pers, nn = host_image_of(dev)          # (the nodes point into `pers`: keep it alive while they are read)
            assert_dumps_equal(oracle.dump_image(nodes, nn), ref.dump(), name)
        nodes, pers, nn = images["A"]
        assert_frame_equals_oracle(A, nodes, nn, ua, "A's frame", 1000)
    finally:
        A.L.simlod_context_attach(B.ctx, B._p(B.nodes))                  # back to its own context: each close() then destroys its own
        B.close()
        A.close()
