"""CPU tier of tests/test_gpu_builder_states.py: what that module holds the device against must stand on its own first.  `collapse` (the
mirrors' first leaves of more than 50 chunks) against brute force and against itself; the oracle twins of the states, each through the
guards the GPU battery uses, with the Shape it uses; the oracle's continuous build that a resumed import of over-full leaves must reach; and
the precondition helpers, each against a hand-made input that does not take the path.  The lasso, the summaries and the inverses (query,
summary, paint) run on the collapsed octree and on every twin with the rest of the battery's mirrors: their guards hold by the references
alone, on the collapsed octree each of them reaches samples behind a leaf's row with the classes the node rules give, and on every twin the
summaries of a selection and of its inverse add up to the whole box's.  Oracle, numpy mirrors and brute force only."""
import numpy as np
import pytest

import cases
import delta_ref
import neighbours_ref as nr
import pack_ref as kr
import paint_ref as pf
import profile_ref as pr
import rays_ref as yr
import region_ref as rr
import states_ref as sr
from simlod_amd import abi
from simlod_amd.octree_io import Region, classify_footprint, classify_lasso, classify_nodes, classify_profile, delta_between
from test_gpu_trunk import _partition

_TWINS, _MIRRORS = {}, {}
SMALL_TWINS = ["G 90000 poisoned", "G 90000 continued", "I B"]          # under 300 000 samples: small enough for one Python loop per sample


def _twin(name):
    if name not in _TWINS:
        _TWINS[name] = sr.twin(name, _partition)
    return _TWINS[name]


def _mirrors(name):
    """The battery's mirrors on a twin (state A with the pair queries' "all" too, as its GPU battery asks); kept for the twins that further
    tests look into."""
    if name in _MIRRORS:
        return _MIRRORS[name]
    ex, pts, box, shape, _ = _twin(name)
    m = sr.mirrors(ex, pts, sr.view_uniforms(box, shape.camera), name, shape, pairs_all=name == "A")
    if name == "A" or name in SMALL_TWINS:
        _MIRRORS[name] = m
    return m


@pytest.fixture(scope="module", autouse=True)
def _release(built_libs):
    yield
    _TWINS.clear()
    _MIRRORS.clear()


# ---- collapse ----------------------------------------------------------------------------------------------------------------------------------
def test_collapse_is_an_octree_of_overfull_leaves_that_holds_the_input(built_libs):
    c, pts, box, shape, ho = _twin("A")
    c.validate(buildable=True)
    sr.assert_state_a(sr.ERR_NODES, c.nodes)
    n = c.nodes["numSamples"][1:]
    assert (int(n.min()), int(n.max())) == (74_517, 75_680) and ((n + 999) // 1000 > sr.ROW).all()      # 75 or 76 chunks: the row and 25 behind it
    rr.assert_same_multiset(c.truncated(20, "cut").samples, pts, "collapse")
    pts3 = np.concatenate(sr.a_input()[2][:3])
    ho3, u3, _ = sr.oracle_build(box, sr.a_input()[2][:3])
    n3 = sr.collapse(sr.export_of(ho3, u3)).nodes["numSamples"][1:]
    assert (int(n3.min()), int(n3.max())) == (55_905, 56_863) and int(n3.sum()) == len(pts3)
    # folding nothing changes nothing; the leaves of a level-1 collapse are the oracle's subtrees
    full = sr.export_of(ho, cases.uniforms_for(box, np.eye(4, dtype=np.float32)))
    deep = sr.collapse(full, 20)
    assert deep.nodes.tobytes() == full.nodes.tobytes() and deep.samples.tobytes() == full.samples.tobytes()
    assert c.nodes["numSamples"][0] == full.nodes["numSamples"][0] and c.samples[: int(c.nodes["numSamples"][0])].tobytes() == full.samples[: int(full.nodes["numSamples"][0])].tobytes()


def test_mirrors_on_the_collapsed_octree_agree_with_brute_force_and_each_other(built_libs):
    c, pts, box, shape, _ = _twin("A")
    m = _mirrors("A")
    q = m["q"]
    for sel in ("cut", "all"):
        table = c.truncated(20, sel)
        hits, cnt = m["rays"][sel]
        assert hits.tobytes() == yr.exhaustive(table, q.rays).tobytes(), f"cast {sel} against the exhaustive search"
        yr.assert_hits_index_export(hits, table, f"cast {sel}")
        nb, within, _ = m["spheres"][sel]
        want, ww = nr.exhaustive(table, q.spheres, sr.K)
        assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww), f"neighbours {sel} against the exhaustive search"
        nr.assert_found_index_export(nb, table, f"neighbours {sel}")
    # hits and neighbours behind the row: ordinals of 50 000 and more
    assert int((m["rays"]["cut"][0]["ordinal"][m["rays"]["cut"][0]["node"] != abi.EXPORT_NONE] >= sr.OVER).sum()) >= 8
    f = m["spheres"]["cut"][0]
    assert int((f["ordinal"][f["node"] != abi.EXPORT_NONE] >= sr.OVER).sum()) >= 64
    # the crops keep whole leaves (the star) and parts of them, and a crop is an octree
    for key, (crop, cnt) in m["crop"].items():
        crop.validate()
    assert int(m["crop"]["footprint", "cut"][1]["numCopiedNodes"]) == 2
    assert int(m["delta"].counts["numKept"]) == 5 and int(m["coarser"][1]["bias"]) == 6


def test_held_counts_around_the_row_end_send_exactly_the_tails(built_libs):
    """A receiver that holds 49 999, 50 000, 50 001 and 56 000 samples of four 75 000-sample leaves: with tails the delta is samples[held:] of
    each — first pieces that begin in chunk 49 (the row's last slot), 50 (the first behind it) and 56 —, without them the leaves come whole."""
    c, pts, box, shape, _ = _twin("A")
    fresh = c.view(sr.view_uniforms(box, "closer"))
    assert int(((fresh.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0).sum()) == 8 and fresh.num_samples == len(pts)
    counts = (49_999, 50_000, 50_001, 56_000)
    held, idx = sr.held_table(fresh, counts)
    assert [int(v) for v in held.nodes["numSamples"][idx]] == list(counts) and [k // 1000 for k in counts] == [49, 50, 50, 56]
    d = delta_between(fresh, held, tails=True)
    delta_ref.assert_delta_consistent(d, held, fresh)
    want = np.concatenate([fresh.samples[int(a) + k: int(a) + int(n)] for a, k, n in zip(fresh.nodes["firstSample"][idx], counts, fresh.nodes["numSamples"][idx])])
    assert d.samples.tobytes() == want.tobytes() and delta_ref.states(d) == (4, 4, 0, 0)
    w = delta_between(fresh, held, tails=False)
    delta_ref.assert_delta_consistent(w, held, fresh)
    assert delta_ref.states(w) == (4, 0, 4, 4) and w.num_samples == int(fresh.nodes["numSamples"][idx].astype(np.int64).sum())


def _result_classes(full, result, region, footprint=None, profile=None, lasso=None):
    """Per entry of a crop's table, by the node rules alone (region rule 2, footprint rules F3 / F4, profile rule P3, lasso rules L2-L4):
    -> (its entry in `full`, whether the node is copied whole, whether it is filtered sample by sample)"""
    key = lambda a: list(zip(a["level"].tolist(), a["X"].tolist(), a["Y"].tolist(), a["Z"].tolist()))
    at = {k: i for i, k in enumerate(key(full.nodes))}
    src = np.array([at[k] for k in key(result.nodes)])
    out, ins = classify_nodes(np.asarray(region.planes, dtype=np.float32).astype(np.float64), full.nodes, full.box_min, full.box_max)
    if footprint is not None:
        near, corner = classify_footprint(footprint, full.nodes, full.box_min, full.box_max)
        out, ins = out | (~near & ~corner), ins & ~near & corner
    if profile is not None:
        far, covered = classify_profile(profile, full.nodes, full.box_min, full.box_max)
        out, ins = out | far, ins & covered
    if lasso is not None:
        behind, covered = classify_lasso(lasso, full.nodes, full.box_min, full.box_max)
        out, ins = out | behind, ins & covered
    return src, ins[src], ~out[src] & ~ins[src]


def test_lasso_summary_and_inverse_on_the_collapsed_octree_reach_behind_the_row(built_libs):
    """What makes state A worth running for the lasso, the summary and the inverse: the screen lasso filters seven leaves of 75 chunks, and
    samples pass at ordinals of 50 000 and more; each summary's contributing samples (the crop's, rule S0) include such samples; each inverse
    paint recolours such samples — in a leaf the inverse copies whole (the lasso leaves one outside: every chunk behind the row is stored, by
    the SET without `previous` too where the selection has such a leaf) and in leaves it filters.  Per node the results' classes are the node
    rules' (_result_classes): what the selection copies the inverse lists at zero samples, what it leaves outside the inverse copies whole."""
    c, pts, box, shape, _ = _twin("A")
    m = _mirrors("A")
    q = m["q"]
    row = sr.ROW * abi.POINTS_PER_CHUNK
    ns = c.nodes["numSamples"].astype(np.int64)
    ex, cnt = m["lasso"]["cut"]
    again, index = c.crop(Region(), 20, "cut", lasso=q.lasso, return_index=True)
    assert again.samples.tobytes() == ex.samples.tobytes() and again.nodes.tobytes() == ex.nodes.tobytes()
    src, copied, filtered = _result_classes(c, ex, Region(), lasso=q.lasso)
    leaf = (ex.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    assert (int((copied & leaf).sum()), int((filtered & leaf).sum())) == (int(cnt["numCopiedNodes"]), int(cnt["numFilteredNodes"])) == (0, 7)
    n, first = ex.nodes["numSamples"].astype(np.int64), ex.nodes["firstSample"].astype(np.int64)
    behind = [int((index[first[t]: first[t] + n[t]] - int(c.nodes["firstSample"][src[t]]) >= row).sum()) for t in np.nonzero(filtered & leaf)[0]]
    assert sum(behind) == sr.behind_row(c, index) and max(behind) >= 1, "no leaf the lasso filters has a passing sample behind the row"
    print(f"lasso on A: passing samples at ordinals >= 50 000 per filtered leaf {behind}")
    for (kind, sel), region, lasso in ((("region", "cut"), q.region, None), (("region", "all"), q.region, None), (("lasso", "cut"), Region(), q.lasso), (("box", "cut"), Region(), None)):
        index = c.crop(region, 20, sel, lasso=lasso, return_index=True)[1]
        assert m["summary"][kind, sel][0].num_samples == len(index) and sr.behind_row(c, index) >= 1, f"summary {kind} {sel}: no contributing sample behind the row"
    state, far = c, {"copied": 0, "filtered": 0}
    for kind, call in zip(sr.selections(q), m["inverse"]["paint"]):
        region, fp, lasso = call.sel3
        res, index = state.crop(region, 20, "all", footprint=fp, lasso=lasso, invert=True, return_index=True)
        assert np.array_equal(state.samples["color"][index], call.previous) and res.nodes.tobytes() == m["inverse"]["query"][kind, "all"][0].nodes.tobytes()
        src, emptied, filtered = _result_classes(c, res, region, fp, lasso=lasso)
        assert np.array_equal(src, np.arange(c.num_nodes))                              # rule I3: every node, in the export's order
        whole = ~emptied & ~filtered
        n = res.nodes["numSamples"].astype(np.int64)
        assert not n[emptied].any() and np.array_equal(n[whole], ns[whole])
        assert (int((whole & (ns > 0)).sum()), int((filtered & (ns > 0)).sum())) == (int(call.counts["numCopiedNodes"]), int(call.counts["numFilteredNodes"]))
        assert sr.behind_row(c, index) >= 1, f"inverse paint {kind}: no recoloured sample behind the row"
        far["copied"] += int((whole & (n > row)).sum())
        far["filtered"] += int(sum(sr.behind_row(c, index[(index >= int(c.nodes["firstSample"][t])) & (index < int(c.nodes["firstSample"][t]) + ns[t])]) > 0 for t in np.nonzero(filtered & (ns > row))[0]))
        state = call.export
    print(f"inverse paint on A: leaves recoloured at a per-node offset >= 50 000: {far}")
    assert far["copied"] >= 1 and far["filtered"] >= 1, far


def test_profile_and_paint_on_the_collapsed_octree_reach_behind_the_row(built_libs):
    """What makes state A worth running for the profile and the paint: items with k >= 50 and offsets of 50 000 and more.  The corridor's cut
    copies leaves of 75 chunks whole (k_pr_write stores chunk k at firstSample + 1000 k) and filters others, and in a filtered leaf samples
    pass whose ordinal in the leaf is 50 000 or more (they lie in chunks the `next` chain reaches, not the row); both paint calls write
    previous[firstSample + offset] with a per-node offset of 50 000 or more — in a copied node (the star's two leaves: offset 1000 k + rank) and
    in a filtered one (offset it.off + rank, the samples that passed before the item)."""
    c, pts, box, shape, _ = _twin("A")
    m = _mirrors("A")
    q = m["q"]
    ex, rec, cnt = m["profile"]["cut"]
    again, index = c.crop(Region(), 20, "cut", profile=q.profile, return_index=True)
    assert again.samples.tobytes() == ex.samples.tobytes() and again.nodes.tobytes() == ex.nodes.tobytes()
    src, copied, filtered = _result_classes(c, ex, Region(), profile=q.profile)
    leaf = (ex.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    n, first = ex.nodes["numSamples"].astype(np.int64), ex.nodes["firstSample"].astype(np.int64)
    assert (int((copied & leaf).sum()), int((filtered & leaf).sum())) == (int(cnt["numCopiedNodes"]), int(cnt["numFilteredNodes"])) == (2, 6)
    assert (n[copied & leaf] == c.nodes["numSamples"][src[copied & leaf]]).all() and (n[copied & leaf] > sr.ROW * abi.POINTS_PER_CHUNK).all()
    behind = [int((index[first[t]: first[t] + n[t]] - int(c.nodes["firstSample"][src[t]]) >= sr.OVER).sum()) for t in np.nonzero(filtered & leaf)[0]]
    assert max(behind) >= 1, "no filtered leaf has a passing sample behind the row"
    print(f"profile on A: passing samples at ordinals >= 50 000 per filtered leaf {behind}, samples per filtered leaf {n[filtered & leaf].tolist()}")
    state, far = c, {"copied": 0, "filtered": 0}
    for call in m["paint"]:
        res, index = state.crop(call.region, 20, "all", footprint=call.footprint, return_index=True)
        assert np.array_equal(state.samples["color"][index], call.previous)              # previous[j] belongs to sample j of the query's order
        src, copied, filtered = _result_classes(c, res, call.region, call.footprint)
        n = res.nodes["numSamples"].astype(np.int64)
        far["copied"] += int((copied & (n > sr.OVER)).sum())
        far["filtered"] += int((filtered & (n > sr.OVER)).sum())
        state = call.export
    print(f"paint on A: nodes with previous at a per-node offset >= 50 000: {far}")
    assert far["copied"] >= 1 and far["filtered"] >= 1, far


@pytest.mark.parametrize("name", SMALL_TWINS)
def test_mirrors_of_paint_and_profile_against_the_per_sample_references(built_libs, name):
    """On the twins small enough for a Python loop per sample: both battery paint calls of OctreeExport.paint against paint_ref.targets and
    paint_ref.paint (target set, order, previous and the colour column after the call), and the segment of every sample OctreeExport.profile
    returns against rule P1 decided exactly — with every sample it does not return in no segment."""
    ex, pts, box, shape, _ = _twin(name)
    assert ex.num_samples < 300_000
    m = _mirrors(name)
    q = m["q"]
    assert pf.in_contract(ex.samples, ex.box_min, ex.box_max)
    state = ex
    for k, call in enumerate(m["paint"]):
        idx = pf.targets(state.samples, call.region.planes, call.footprint)
        col, prev = pf.paint(state.samples, idx, call.paint.record(), call.colors)
        assert len(idx) == int(call.counts["numSamples"]) > 0, f"{name} call {k + 1}"
        assert np.array_equal(np.asarray(prev, np.uint32), call.previous), f"{name} call {k + 1}: previous"
        assert np.array_equal(col, call.export.samples["color"]), f"{name} call {k + 1}: the colours after the call"
        assert all(call.export.samples[a].tobytes() == state.samples[a].tobytes() for a in "xyz")
        state = call.export
    mirror, rec, cnt = m["profile"]["all"]
    seg = pr.locate_exact(q.profile, mirror.samples)
    assert (seg >= 0).all() and np.array_equal(rec["segment"].astype(np.int64), seg), f"{name}: a returned sample's segment"
    assert int((pr.locate_exact(q.profile, ex.samples) >= 0).sum()) == mirror.num_samples, f"{name}: a sample in the corridor was not returned"


def test_packed_tails_around_the_row_end_merge_within_the_bound(built_libs):
    """The tails delta of test_held_counts_around_the_row_end_send_exactly_the_tails, packed: GROWN ranges that begin at 49 999, 50 000, 50 001
    and 56 000 of leaves of 75 000 points.  The words at both ends of every range are pack_ref's record by record; unpacked and merged into the
    held table the delta gives the exact merge's table, its voxel entries bit for bit, its leaf entries within rule K8's bound."""
    c, pts, box, shape, _ = _twin("A")
    fresh = c.view(sr.view_uniforms(box, "closer"))
    counts = (49_999, 50_000, 50_001, 56_000)
    held, idx = sr.held_table(fresh, counts)
    d = delta_between(fresh, held, tails=True)
    assert delta_ref.states(d) == (4, 4, 0, 0)
    pd, pc = d.pack(return_counts=True)
    assert (int(pc["numSamples"]), int(pc["numInexact"]), int(pc["numAlpha"]), int(pc["error"])) == (d.num_samples, 0, 0, 0)
    ends = {i for t, f, n in kr.ranges(d.nodes, d.entries) for i in (f, f + 1, f + n - 1)}
    want = kr.pack_ref(d.nodes, d.samples, d.box_min, d.box_max, d.entries, pick=ends)
    assert len(want) == len(ends) == 12 and all(int(pd.packed[i]) == int(w[0]) for i, w in want.items())
    back = pd.unpack()
    assert back.entries.tobytes() == d.entries.tobytes() and back.nodes.tobytes() == d.nodes.tobytes()
    exact, lossy = d.apply(held), back.apply(held)
    assert lossy.nodes.tobytes() == exact.nodes.tobytes() == fresh.nodes.tobytes() and exact.samples.tobytes() == fresh.samples.tobytes()
    vox = kr.voxel_mask(exact.nodes, exact.num_samples)
    assert lossy.samples[vox].tobytes() == exact.samples[vox].tobytes()
    n, worst = kr.assert_points_within_bound(exact.nodes, exact.samples, lossy.samples, exact.box_min, exact.box_max, what="merged leaf entries")
    assert n == int((~vox).sum()) == len(pts) and (lossy.samples["color"] == exact.samples["color"]).all()
    # the heads are the receiver's own and stay exact, the tails moved
    for t, k in zip(idx, counts):
        a = int(exact.nodes["firstSample"][t])
        assert lossy.samples[a: a + k].tobytes() == exact.samples[a: a + k].tobytes()
        assert lossy.samples[a + k: a + int(exact.nodes["numSamples"][t])].tobytes() != exact.samples[a + k: a + int(exact.nodes["numSamples"][t])].tobytes()


# ---- the oracle twins of the states ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E1", "E2", "E3", "E4", "E5", "F", "H", "D hotspot_150k", "D dense_cube", "G 600000 poisoned", "G 600000 continued",
                                  "G 90000 poisoned", "G 90000 continued", "I A", "I B"])
def test_oracle_twin_passes_the_guards_of_its_state(built_libs, name):
    """The battery's mirrors on the oracle's octree of the state's input, with the Shape the GPU tier passes: every guard holds, the cuts are
    the brute-force filters, t and d2 are the brute force's; the lasso's and the inverses' cuts are the exact rules' over the points, the
    summaries summary_ref's, and the summaries of a selection and of its inverse add up to the whole box's field by field (rules I6 / I7).
    (E1 .. E5: whatever number of batches a launch under the time budget takes.)"""
    ex, pts, box, shape, ho = _twin(name)
    ex.validate(buildable=True)
    rr.assert_same_multiset(ex.truncated(20, "cut").samples, pts, name)
    m = _mirrors(name)
    print(f"{name}: the lasso copies {int(m['lasso']['cut'][1]['numCopiedNodes'])} leaves and filters {int(m['lasso']['cut'][1]['numFilteredNodes'])}; "
          f"leaves the inverses empty / copy whole: {m['inverse']['classes']}")
    q = m["q"]
    foot = ex.summarize(Region(), 20, "cut", footprint=q.footprint, z0=q.z0, scale=q.scale)
    sr.assert_halves_add_up(foot, m["inverse"]["summary"]["footprint", "cut"][0], m["summary"]["box", "cut"][0], f"{name}: the footprint's halves")
    if name == "H":
        allpts, _, mask, mine, _ = sr.h_input(_partition)
        assert sr.assert_forced_empty_listed(ex, m["inverse"], allpts, mine, box) >= 1
    if name.startswith("E"):
        # the inverse summary the GPU tier enqueues directly behind the launch is of the BOX's oblique half-space (the host does not know yet
        # which batches the launch took): whatever it took, that inverse holds some of the samples and not all
        cnt = ex.crop(rr.region("oblique", box), 20, "all", return_counts=True, invert=True)[1]
        assert 0 < int(cnt["numSamples"]) < ex.num_samples, f"{name}: {int(cnt['numSamples'])} of {ex.num_samples} samples outside the box's oblique half-space"


def test_twin_of_e_is_the_octree_of_two_of_six_batches(built_libs):
    ex, pts, box, _, ho = _twin("E2")
    st = ho.stats[0]
    sr.assert_stopped_short(st, 2, len(sr.e_input()[2]) - 2)
    assert len(pts) == 200_000 == int(st["numPoints"]) and ex.num_nodes == 41


def test_twin_of_f_stops_at_the_guard_between_the_first_and_the_third_batch(built_libs):
    pts, box, batches = sr.f_input()
    cap, after = sr.f_capacity(box, batches)
    assert after[0] + 200_000_000 < cap < after[1] + 200_000_000        # the second batch is let in, the third is not
    ex, held, _, _, ho = _twin("F")
    sr.assert_stopped_short(ho.stats[0], 2, 2, guard=True)
    assert len(held) == 1_000_000 and int(ho.stats["allocatedBytes_persistent"][0]) == after[1]


def test_twin_of_h_has_nodes_the_mask_forces(built_libs):
    pts, box, mask, mine, batches = sr.h_input(_partition)
    ex, _, _, _, _ = _twin("H")
    assert sr.assert_masked_rank(ex.nodes, pts, mine, box, mask) == 9
    # ... and half the points are too few: the mask of 300 000 names nodes that every rank splits anyway
    p2, b2, m2, mine2, bt2 = sr.h_input(_partition, 300_000)
    ho2, u2, _ = sr.oracle_build(b2, bt2, mask=m2)
    with pytest.raises(AssertionError, match="forces nothing"):
        sr.assert_masked_rank(sr.export_of(ho2, u2).nodes, p2, mine2, b2, m2)


def test_twin_of_b_is_the_level_2_octree_the_resume_must_reach(built_libs):
    pts, box, more = sr.b_input()
    ho, u, _ = sr.oracle_build(box, sr.a_input()[2] + more)
    ex = sr.export_of(ho, u)
    sr.assert_no_overfull(ex.nodes)
    t = ex.nodes
    leaf = (t["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    assert ex.num_nodes == 73 and [int((t["level"] == l).sum()) for l in range(3)] == [1, 8, 64]
    assert not leaf[t["level"] < 2].any() and leaf[t["level"] == 2].all() and int(t["numSamples"][leaf].sum()) == 800_000
    # every one of the 200 000 resumed points' octants is touched
    octant = (pts["x"][600_000:] >= 0.5).astype(int) * 4 + (pts["y"][600_000:] >= 0.5).astype(int) * 2 + (pts["z"][600_000:] >= 0.5).astype(int)
    assert len(np.unique(octant)) == 8


# ---- the precondition helpers reject what does not take the path ---------------------------------------------------------------------------------
def test_precondition_helpers_reject_octrees_off_the_path(built_libs):
    c, pts, box, _, ho = _twin("A")
    sr.assert_state_a(sr.ERR_NODES, c.nodes)
    with pytest.raises(AssertionError):
        sr.assert_state_a(0, c.nodes)                                    # no error bit: the node array was not full
    uncollapsed = _twin("D dense_cube")[0]
    with pytest.raises(AssertionError):
        sr.assert_state_a(sr.ERR_NODES, uncollapsed.nodes)               # 73 nodes: the splits went through
    small = c.nodes.copy()
    small["numSamples"][3] = sr.OVER                                     # a leaf that is exactly full has nothing pending
    with pytest.raises(AssertionError):
        sr.assert_state_a(sr.ERR_NODES, small)
    with pytest.raises(AssertionError):
        sr.assert_no_overfull(c.nodes)
    sr.assert_no_overfull(uncollapsed.nodes)
    # state C: the spill bit alone, a pending leaf beside a split one
    mixed = uncollapsed.nodes.copy()
    first_leaf = int(np.nonzero((mixed["flags"] & abi.EXPORT_FLAG_LEAF) != 0)[0][0])
    mixed["numSamples"][first_leaf] = sr.OVER + 1
    assert sr.assert_state_c(sr.ERR_SPILLED, mixed) == 1
    for dbg, table in ((0, mixed), (sr.ERR_SPILLED | sr.ERR_NODES, mixed), (sr.ERR_SPILLED, uncollapsed.nodes), (sr.ERR_SPILLED, c.nodes[:1])):
        with pytest.raises(AssertionError):
            sr.assert_state_c(dbg, table)
    # a launch that stopped short
    st = np.zeros(1, dtype=abi.stats_dtype)[0]
    st["batchletIndex"] = 2
    sr.assert_stopped_short(st, 2, 4)
    for taken, pending, guard in ((3, 3, False), (2, 0, False), (2, 4, True)):
        with pytest.raises(AssertionError):
            sr.assert_stopped_short(st, taken, pending, guard)
    # the guards
    with pytest.raises(AssertionError):
        sr.coarser_budget([600_000, 600_000, 600_000, 0, 0])
    assert sr.coarser_budget([9, 9, 5, 7, 0]) == (5, 2)
    cnt = np.zeros((), dtype=abi.query_counts_dtype)
    cnt["numSamples"], cnt["numCandidates"], cnt["numFilteredNodes"] = 5, 10, 3
    sr.assert_crop_not_vacuous(cnt, "hand-made", copies=False)
    with pytest.raises(AssertionError):
        sr.assert_crop_not_vacuous(cnt, "hand-made")
    cnt["numCopiedNodes"], cnt["numSamples"] = 1, 10
    with pytest.raises(AssertionError):
        sr.assert_crop_not_vacuous(cnt, "hand-made")
    # behind the row: ordinal 49 999 of a leaf is in the row's last chunk, 50 000 in the first behind it; an inner node's voxels never count
    a = int(c.nodes["firstSample"][1])
    assert [sr.behind_row(c, [i]) for i in (0, a + 49_999, a + 50_000, a + int(c.nodes["numSamples"][1]) - 1)] == [0, 0, 1, 1]
    # halves that do not add up, a summary that is not the selection's, a forced node that is not empty
    m = _mirrors("A")
    pos, inv, whole = m["summary"]["region", "cut"][0], m["inverse"]["summary"]["region", "cut"][0], m["summary"]["box", "cut"][0]
    sr.assert_halves_add_up(pos, inv, whole, "hand-made")
    with pytest.raises(AssertionError):
        sr.assert_halves_add_up(pos, pos, whole, "hand-made")
    with pytest.raises(AssertionError):
        sr.assert_summary_is_exact(pos, pts[sr.rr.brute_mask(m["q"].region, pts)][1:], c, m["q"], "hand-made")
    with pytest.raises(AssertionError, match="holds samples"):
        sr.assert_forced_empty_listed(c, m["inverse"], pts, pts[:1], box)       # (every node of A holds samples)
