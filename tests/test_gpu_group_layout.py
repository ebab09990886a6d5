"""The default exact group of five batches fits the reference host's 300 MB momentary buffer (construct.hip layout_construct): with
default knobs a launch that finds five batches takes them as ONE group, one that finds six as groups of five and one — and the octree is the port
oracle's: the whole dump, the build fields of Stats, the structural invariants (compared the way tests/test_gpu_groups.py compares)."""
import pytest

import oracle
from cases import H, W
from simlod_amd import synthetic
from test_gpu_groups import GROUP_PERSISTENT, _cam, _compare
from test_gpu_parity import _device

pytestmark = pytest.mark.gpu

REFERENCE_HOST_MOMENTARY = 300_000_000
BATCH = 30_000


@pytest.mark.parametrize("num_batches,groups", [(5, 1), (6, 2)])
def test_default_groups_of_five_fit_the_reference_hosts_momentary_buffer(built_libs, num_batches, groups):
    pts, box = synthetic.uniform_cube(num_batches * BATCH, seed=77)
    batches = [pts[i:i + BATCH] for i in range(0, len(pts), BATCH)]
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=REFERENCE_HOST_MOMENTARY)      # default knobs: SIMLOD_EXACT_GROUP is not set
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        ref = oracle.HostOctree("port", persistent_bytes=GROUP_PERSISTENT)
        ref.reset(u)
        for b in batches:
            ref.upload(b)
            ref.construct(u)
        assert ref.last_error() == 0 and int(ref.stats["batchletIndex"][0]) == num_batches
        dev.reset(u)
        dev.groups_ingested(zero=True)
        for b in batches:
            dev.upload(b)
        dev.set_batch_limit(num_batches)
        dev.construct(u)                                   # ONE launch
        assert dev.processed() == num_batches, "the launch took every pending batch"
        assert dev.group_size() == 5, "the layout of the 300 MB buffer holds the default group of five"
        assert dev.groups_ingested() == groups, f"{num_batches} batches: groups of five, then the rest"
        nodes, pers, nn = _compare(dev, f"{num_batches} batches in 300 MB", ref)
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()
