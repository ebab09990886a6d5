"""Shared by the inverse-selection tests (include/simlod_hip.h, "inverse selections"): the selections they use, family by family, rule I1 said
once more in Python — a mask over an export's samples, sample by sample, with no node shortcut — and the class map of rule I2 in numpy."""
import numpy as np

import cases
import footprint_ref as fr
import lasso_ref as lr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Lasso, Region

W, H = cases.W, cases.H
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
OUTSIDE, FILTERED, COPIED, EMPTIED = 0, 1, 2, 3
FAMILIES = ["planes", "footprint", "lasso"]
# the selections for which the POSITIVE mirror must report filtered, copied and unlisted nodes at ALL@20 (test_inverse_rules.py asserts it):
# without a copied node of the positive query no node of the inverse is EMPTIED
ALL_CLASSES = [("planes", "terrain_4x100k", "oblique"), ("planes", "hotspot_150k", "box"), ("footprint", "hotspot_150k", "rect"),
               ("lasso", "terrain_4x100k", "half"), ("lasso", "hotspot_150k", "rect_fp")]


def half_screen(T):
    """The left half of the test screen of the camera T: with the bird camera it swallows whole nodes, cuts others and leaves the rest."""
    return Lasso.from_pixels(T, W, H, [(0, 0), (W / 2, 0), (W / 2, H), (0, H)])


def names_for(family, case):
    """The named selections of a family for a case; star128 stays off the cases it is slow on, as in lasso_ref / footprint_ref."""
    if family == "planes":
        return list(rr.REGION_NAMES)
    if family == "footprint":
        return fr.names_for(case)
    return lr.names_for(case) + ["half", "rect_fp"]


def selection(family, kind, box, box_min=(0, 0, 0)):
    """-> (region, footprint or None, lasso or None).  The lassos go with the bird camera."""
    if family == "planes":
        return rr.region(kind, box, box_min), None, None
    if family == "footprint":
        return Region(), fr.footprint(kind, box, box_min), None
    T = lr.transform("bird", box, box_min)
    if kind == "half":
        return Region(), None, half_screen(T)
    if kind == "rect_fp":
        return Region(), None, Lasso.from_footprint(fr.footprint("rect", box, box_min))
    return Region(), None, lr.lasso(kind, T)


def class_map(outside, inside):
    """Rule I2 from the positive query's two masks: outside -> COPIED, copied -> EMPTIED, else FILTERED."""
    return np.where(outside, COPIED, np.where(inside, EMPTIED, FILTERED))


def passes_inverse(region, footprint, lasso, samples):
    """Rule I1, sample by sample: not (region rule 3 and, where given, F1 or L1 decided exactly)."""
    with np.errstate(invalid="ignore"):
        ok = rr.brute_mask(region, samples)
    if footprint is not None:
        ok &= fr.contains_exact(footprint, samples)
    if lasso is not None:
        ok &= lr.contains_exact(lasso, samples)
    return ~ok


def selected_ranges(full, ml, sel):
    """Per entry of simlod_export_octree(ml, sel)'s table, the range of its samples in the FULL export (empty for an entry that is not selected)."""
    t = full.truncated(ml, sel).nodes
    src = full.nodes[: len(t)]
    chosen = (t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
    first = src["firstSample"].astype(np.int64)
    return [(int(first[k]), int(first[k]) + (int(src["numSamples"][k]) if chosen[k] else 0)) for k in range(len(t))]


def inverse_per_node(full, mask, ml, sel):
    """The inverse's samples per table entry from the mask of passes_inverse over the full export's samples."""
    smp = full.samples
    return [smp[a:b][mask[a:b]] for a, b in selected_ranges(full, ml, sel)]
