"""Seeded parity cases shared by the golden generator, the oracle pin tests and the GPU parity tests."""
import numpy as np

from simlod_amd import abi, camera, synthetic

W = H = 256


def _cam(box):
    return camera.lookat_transform((1.8 * box[0], -1.2 * box[1], 1.4 * max(box)), (0.5 * box[0], 0.5 * box[1], 0.3 * box[2]), W, H)


def case(name):
    """-> (points, box, batch, transform)"""
    if name == "uniform_3x40k":            # root splits in batch 2 with 40 000 stored points -> spill copy + chunk recycling
        pts, box = synthetic.uniform_cube(120_000, seed=1)
        return pts, box, 40_000, _cam(box)
    if name == "hotspot_150k":             # every point in one level-3 cell: 4+ expand rounds inside one batch
        pts, box = synthetic.hotspot(150_000, seed=11, level=3, cell=(5, 2, 6))
        return pts, box, 150_000, _cam(box)
    if name == "terrain_4x100k":           # swath-ordered surface, ragged leaf populations, several split generations
        pts, box = synthetic.terrain(400_000, seed=3, box=(600.0, 400.0, 40.0), tile=50.0)
        return pts, box, 100_000, _cam(box)
    if name == "ragged_tiny":              # batches of 1, 7 and 49 999 + an EMPTY batch, then the 50 001st point
        pts, box = synthetic.uniform_cube(50_010, seed=5)
        return pts, box, None, _cam(box)   # batch boundaries: see ragged_batches()
    raise KeyError(name)


CASES = ["uniform_3x40k", "hotspot_150k", "terrain_4x100k", "ragged_tiny"]


def batches_of(name, pts, batch):
    if name == "ragged_tiny":
        cuts = [0, 1, 8, 8, 50_000, 50_001, 50_010]      # 1, 7, 0 (empty), 49 992, 1 (crosses the 50 000 limit), 9
        return [pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return [pts[i:i + batch] for i in range(0, len(pts), batch)]


def uniforms_for(box, T, *, hqs=False, persistent=1 << 30, momentary=300_000_000, point_size=1, box_min=(0.0, 0.0, 0.0)):
    return abi.make_uniforms(W, H, T, box, persistent_capacity=persistent, momentary_capacity=momentary, hqs=hqs, point_size=point_size, box_min=box_min)


# ---- a box off the origin ----------------------------------------------------------------------------------------------------------------
# Named offsets: `dyadic` shifts exactly and with mixed signs, `inexact` makes boxMax - boxMin differ from the box size,
# `georef` quantises the coordinates to 1/32 and 1/2 so that min + X * nodeSize rounds at every level.
DYADIC = (0.25, -3.5, 100.0)
INEXACT_UNIT = (3.3, -7.7, 0.1)
INEXACT_TERRAIN = (1000.3, -2000.7, 33.1)
GEOREF = (512345.75, 4187654.5, 12.125)


def offset_of(kind, box):
    """The named offset for a box: `inexact` depends on the box's size, `georef` goes with the 600 x 400 x 40 terrain only."""
    big = float(max(box)) > 2.0
    if kind == "dyadic":
        return DYADIC
    if kind == "inexact":
        return INEXACT_TERRAIN if big else INEXACT_UNIT
    if kind == "georef":
        assert big, "georef goes with the terrain box"
        return GEOREF
    raise KeyError(kind)


def shift_points(pts, offset):
    """A copy of `pts` with float32(p + offset) per axis: simply a new input (no exactness of the shift is assumed)."""
    out = np.array(pts, dtype=abi.point_dtype, copy=True)
    for k, a in enumerate("xyz"):
        out[a] = pts[a] + np.float32(offset[k])
    return out


def shifted(name, offset):
    """-> (points, box_min, box_size, batch): the case's points moved by `offset`.  fp32 rounding is monotone, so every point stays inside
    [boxMin, boxMax] = [float32(offset), float32(offset) + box_size]."""
    pts, box, batch, _ = case(name)
    return shift_points(pts, offset), tuple(float(np.float32(v)) for v in offset), box, batch


def shifted_cam(box, offset, width=W, height=H):
    """The cases' camera translated by `offset`."""
    o = np.asarray(offset, dtype=np.float64)
    eye = np.array([1.8 * box[0], -1.2 * box[1], 1.4 * max(box)]) + o
    target = np.array([0.5 * box[0], 0.5 * box[1], 0.3 * box[2]]) + o
    return camera.lookat_transform(tuple(eye), tuple(target), width, height)


def size_differs(u):
    """True where (boxMin + size) - boxMin != size on some axis for the uniforms' own fp32 numbers: the colour filter's octreeSize then
    differs from the cube size."""
    mn, mx = np.asarray(u["boxMin"], np.float32).reshape(3), np.asarray(u["boxMax"], np.float32).reshape(3)
    d = mx - mn
    size = d.max()
    return bool((((mn + size) - mn) != size).any())


def origin_box_uniforms(u):
    """The same uniforms with boxMin = 0 and boxMax unchanged: what a kernel that ignores boxMin would in effect compute with."""
    v = np.array(u, copy=True)
    v["boxMin"] = 0.0
    return v


# ---- a frozen visibility camera: transform_updateBound chooses the nodes, transform draws them -----------------------------------------------
LIVE_CAMERAS = ["panned", "closer", "grazing", "inside", "away", "narrow"]


def camera_pose(which, box, offset=(0.0, 0.0, 0.0), terrain_seed=3):
    """(eye, target) of the named cameras for a box of size `box` at `offset`.  `grazing` skims the synthetic terrain (600 x 400 x 40 box only)."""
    b = np.asarray(box, dtype=np.float64)
    eye, target = np.array([1.8 * b[0], -1.2 * b[1], 1.4 * b.max()]), np.array([0.5 * b[0], 0.5 * b[1], 0.3 * b[2]])
    if which == "bird":
        pass
    elif which == "panned":                 # same eye, the target a box width further along x
        target = target + np.array([b[0], 0.0, 0.0])
    elif which == "closer":                 # half the distance
        eye = target + 0.5 * (eye - target)
    elif which == "inside":
        eye, target = np.array([0.52, 0.48, 0.5]) * b, np.array([0.9, 0.6, 0.45]) * b
    elif which == "away":                   # the bird's eye, looking the other way
        target = eye + (eye - target)
    elif which in ("grazing", "grazing_back"):
        ex, ey = 0.5 * float(b[0]), 0.3 * float(b[1])
        ground = float(synthetic.terrain_height(ex, ey, seed=terrain_seed, box=(600.0, 400.0, 40.0)))
        eye, target = np.array([ex, ey, ground + 6.0]), np.array([ex + 20.0, ey + 200.0, ground - 4.0])
        if which == "grazing_back":         # 30 m back along the view direction
            d = (target - eye) / np.linalg.norm(target - eye)
            eye, target = eye - 30.0 * d, target - 30.0 * d
    else:
        raise KeyError(which)
    o = np.asarray(offset, dtype=np.float64)
    return tuple(eye + o), tuple(target + o)


def frozen_pair(case_name, box, width, height, offset=(0.0, 0.0, 0.0)):
    """(live transform, frozen transform) of a frozen-camera case: the bird camera chooses and `case_name` draws, except `narrow` (the closer
    camera chooses, the bird draws) and `grazing_back` (the grazing camera moved 30 m back chooses, the grazing camera draws)."""
    live, frozen = {"narrow": ("bird", "closer"), "grazing_back": ("grazing", "grazing_back")}.get(case_name, (case_name, "bird"))
    return tuple(camera.lookat_transform(*camera_pose(w, box, offset), width, height) for w in (live, frozen))
