"""Host side of the loader row: LAS / .simlod files -> batches for the ring.

Mirrors the reference's loader interface — `LasHeader` + `load_header` (modules/progressive_octree/LasLoader.h:8-55),
the byte range a loader thread reads for a batch (LasLoader.cpp:147-166: offsetToPointData + bytesPerPoint * firstPoint,
bytesPerPoint * numPoints), the .simlod layout (24-byte header + 16-byte records, main_progressive_octree.cpp:925-929,
tools/las2simlod.mjs:96-147) — but does not parse points on the CPU: the raw records go to the device and
`simlod_decode_las` (simlod_amd/csrc/loader.hip) writes the XYZRGBA points into the ring.  LAZ (laszip) is out of scope.

`write_las` / `las_records` build synthetic LAS files for tests and benchmarks (there is no network for real ones).
"""
import dataclasses
import struct

import numpy as np

from . import abi

# RGB byte offset inside a point record, for the formats the reference takes colour from (LasLoader.cpp:177-185)
RGB_OFFSET = {2: 20, 3: 28, 5: 28, 7: 30}
# ... and of every format that carries the triple (the styled decode's RGB, and what las_records plants)
RGB_OFFSET_ALL = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}
# minimum record length of the LAS point data record formats 0-10 (ASPRS LAS 1.4 R15, tables 7-17)
FORMAT_BYTES = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}


@dataclasses.dataclass
class LasHeader:
    """Same fields as the reference's LasHeader (LasLoader.h:8-19)."""
    versionMajor: int = 0
    versionMinor: int = 0
    headerSize: int = 0
    offsetToPointData: int = 0
    format: int = 0
    bytesPerPoint: int = 0
    numPoints: int = 0
    scale: tuple = (0.0, 0.0, 0.0)
    offset: tuple = (0.0, 0.0, 0.0)
    min: tuple = (0.0, 0.0, 0.0)
    max: tuple = (0.0, 0.0, 0.0)


def load_header(path):
    """loadHeader, LasLoader.h:21-55: fixed byte offsets into the first 375 bytes; the legacy 32-bit point count for
    LAS <= 1.3, the 64-bit one at byte 247 otherwise."""
    with open(path, "rb") as f:
        b = f.read(375).ljust(375, b"\0")
    h = LasHeader()
    h.versionMajor, h.versionMinor = b[24], b[25]
    h.headerSize = struct.unpack_from("<H", b, 94)[0]
    h.offsetToPointData = struct.unpack_from("<I", b, 96)[0]
    h.format = b[104]
    h.bytesPerPoint = struct.unpack_from("<H", b, 105)[0]
    if h.versionMajor == 1 and h.versionMinor <= 3:
        h.numPoints = struct.unpack_from("<I", b, 107)[0]
    else:
        h.numPoints = struct.unpack_from("<Q", b, 247)[0]
    d = lambda o: struct.unpack_from("<d", b, o)[0]
    h.scale = (d(131), d(139), d(147))
    h.offset = (d(155), d(163), d(171))
    h.max = (d(179), d(195), d(211))
    h.min = (d(187), d(203), d(219))
    return h


def read_records(path, header, first, count):
    """The bytes a loader thread reads for one batch (LasLoader.cpp:147-166), as a uint8 array."""
    count = max(0, min(count, header.numPoints - first))
    with open(path, "rb") as f:
        f.seek(header.offsetToPointData + header.bytesPerPoint * first)
        return np.fromfile(f, dtype=np.uint8, count=header.bytesPerPoint * count)


def decode_offset(header, translation):
    """offset_x = header.offset[0] + translation[0] ... (LasLoader.cpp:197-199), in fp64."""
    return tuple(float(np.float64(o) + np.float64(t)) for o, t in zip(header.offset, translation))


def batches(header, batch=abi.MAX_BATCH_SIZE):
    """(first, count) of every batch of a file, as main_progressive_octree.cpp:893-910 queues them."""
    return [(f, min(batch, header.numPoints - f)) for f in range(0, header.numPoints, batch)]


def read_simlod(path):
    """(points, box_size): the 24-byte header holds min (zeros) and max = box size as 6 float32."""
    with open(path, "rb") as f:
        hdr = np.frombuffer(f.read(24), dtype=np.float32)
        pts = np.frombuffer(f.read(), dtype=abi.point_dtype)
    return pts, (hdr[3:6] - hdr[0:3]).astype(np.float32)


def las_records(xyz_int, rgb16, fmt, bytes_per_point=None, seed=0, attributes=None):
    """Raw point records (uint8 [n, bytesPerPoint]) of LAS point format `fmt`: int32 X,Y,Z at bytes 0-11, RGB16 where the
    format has it, every other byte pseudo-random (intensity, flags, gps time, extra bytes ... — a decoder must ignore them).
    attributes: {name (abi.LAS_ATTRIBUTES): values} written into their fields afterwards (a bit field keeps the byte's other bits)."""
    n = len(xyz_int)
    bpp = FORMAT_BYTES[fmt] if bytes_per_point is None else bytes_per_point
    rec = np.random.RandomState(seed).randint(0, 256, size=(n, bpp), dtype=np.uint8)
    rec[:, 0:12] = np.ascontiguousarray(xyz_int.astype("<i4")).view(np.uint8).reshape(n, 12)
    off = RGB_OFFSET_ALL.get(fmt)
    if off is not None and rgb16 is not None:
        rec[:, off:off + 6] = np.ascontiguousarray(rgb16.astype("<u2")).view(np.uint8).reshape(n, 6)
    for name, values in (attributes or {}).items():
        off, kind, shift, mask = las_field(name, fmt)
        if kind == "f8":
            rec[:, off:off + 8] = np.ascontiguousarray(np.asarray(values, "<f8")).view(np.uint8).reshape(n, 8)
            continue
        size = int(kind[1])
        raw = (np.asarray(values).astype(np.int64) & mask) << shift
        old = np.ascontiguousarray(rec[:, off:off + size]).view(f"<u{size}").reshape(n).astype(np.int64)
        new = ((old & ~(mask << shift)) | raw).astype(f"<u{size}")
        rec[:, off:off + size] = np.ascontiguousarray(new).view(np.uint8).reshape(n, size)
    return rec


# ---- colour by attribute (include/simlod_hip.h, "styled decode") ------------------------------------------------------------------------

def las_field(attribute, fmt):
    """(byte offset, kind, shift, mask) of a scalar attribute in a record of format `fmt` (ASPRS LAS 1.4 R15, tables 7-17): kind "u1" / "u2" /
    "i1" / "i2" / "f8"; the value is sign_extend((field >> shift) & mask).  ValueError: the format has no such attribute."""
    a = abi.LAS_ATTRIBUTES[attribute] if isinstance(attribute, str) else int(attribute)
    if not 0 <= fmt <= 10:
        raise ValueError(f"LAS point format {fmt}")
    ext = fmt >= 6
    if a == abi.LAS_INTENSITY:
        return 12, "u2", 0, 0xffff
    if a == abi.LAS_RETURN_NUMBER:
        return 14, "u1", 0, 0xf if ext else 0x7
    if a == abi.LAS_NUMBER_OF_RETURNS:
        return 14, "u1", 4 if ext else 3, 0xf if ext else 0x7
    if a == abi.LAS_CLASSIFICATION:
        return (16, "u1", 0, 0xff) if ext else (15, "u1", 0, 0x1f)
    if a == abi.LAS_USER_DATA:
        return 17, "u1", 0, 0xff
    if a == abi.LAS_SCAN_ANGLE:
        return (18, "i2", 0, 0xffff) if ext else (16, "i1", 0, 0xff)
    if a == abi.LAS_POINT_SOURCE_ID:
        return 20 if ext else 18, "u2", 0, 0xffff
    if a == abi.LAS_GPS_TIME and fmt not in (0, 2):
        return 22 if ext else 20, "f8", 0, 0
    raise ValueError(f"LAS point format {fmt} has no attribute {attribute}")


def _ramp(stops):
    """256 colour words (0x00BBGGRR) through `stops` (r, g, b), evenly spaced, by integer linear interpolation."""
    lut = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        pos = i * (len(stops) - 1)
        seg = min(pos // 255, len(stops) - 2)
        f = pos - seg * 255
        r, g, b = ((stops[seg][k] * (255 - f) + stops[seg + 1][k] * f + 127) // 255 for k in range(3))
        lut[i] = r | (g << 8) | (b << 16)
    return lut


# this project's own tables: control colours (r, g, b) of the ramps, and the colour of each ASPRS class
RAMPS = {
    "gray": [(0, 0, 0), (255, 255, 255)],
    "terrain": [(24, 60, 110), (46, 120, 70), (150, 170, 80), (170, 120, 70), (245, 245, 240)],       # water's edge, meadow, scrub, rock, snow
    "heat": [(10, 10, 60), (140, 20, 120), (230, 90, 30), (255, 230, 120)],
}
CLASS_FALLBACK = (200, 60, 200)
CLASS_COLOURS = {
    0: (110, 110, 110), 1: (170, 170, 170),                     # never classified, unclassified
    2: (150, 105, 60),                                           # ground
    3: (150, 200, 90), 4: (70, 160, 60), 5: (20, 100, 40),       # low, medium, high vegetation
    6: (215, 70, 50),                                            # building
    7: (255, 0, 255), 18: (255, 0, 255),                         # low / high noise
    9: (50, 110, 220),                                           # water
    10: (90, 80, 100), 11: (60, 60, 70),                         # rail, road surface
    13: (240, 200, 40), 14: (240, 170, 40), 15: (200, 140, 30), 16: (240, 220, 120),     # wire guard, conductor, tower, connector
    17: (120, 130, 150),                                         # bridge deck
}


@dataclasses.dataclass
class Style:
    """How a decode colours its points: the attribute, the window [lo, hi) mapped onto the table, and the table (256 x 0x00BBGGRR).
    The SimlodLasStyle of include/simlod_hip.h; the colour rule is stated there and restated by decode_records."""
    attribute: int
    lo: float = 0.0
    hi: float = 256.0
    lut: np.ndarray = None

    def __post_init__(self):
        self.attribute = abi.LAS_ATTRIBUTES[self.attribute] if isinstance(self.attribute, str) else int(self.attribute)
        self.lut = _ramp(RAMPS["gray"]) if self.lut is None else np.ascontiguousarray(self.lut, dtype=np.uint32).reshape(256)

    @classmethod
    def of(cls, attribute, lo, hi, ramp="gray"):
        return cls(attribute, float(lo), float(hi), _ramp(RAMPS[ramp]) if isinstance(ramp, str) else ramp)

    @classmethod
    def rgb(cls):
        return cls(abi.LAS_RGB)

    @classmethod
    def intensity(cls, lo=0, hi=65536, ramp="gray"):
        return cls.of(abi.LAS_INTENSITY, lo, hi, ramp)

    @classmethod
    def classification(cls, palette=None):
        """The class byte indexes the table with itself.  palette: {class: (r, g, b)} over CLASS_COLOURS."""
        colours = {**CLASS_COLOURS, **(palette or {})}
        rgb = [colours.get(c, CLASS_FALLBACK) for c in range(256)]
        return cls(abi.LAS_CLASSIFICATION, 0.0, 256.0, np.array([r | (g << 8) | (b << 16) for r, g, b in rgb], dtype=np.uint32))

    @classmethod
    def elevation(cls, lo, hi, ramp="terrain"):
        """lo, hi: heights in the file's world units (DeviceOctree.upload_las moves them into the decode's frame)."""
        return cls.of(abi.LAS_ELEVATION, lo, hi, ramp)

    @classmethod
    def auto(cls, header):
        """RGB when the header's format has it, grey intensity otherwise."""
        return cls.rgb() if header.format in RGB_OFFSET_ALL else cls.intensity()

    def in_frame(self, translation):
        """This style in the frame a decode with `translation` writes: an elevation window moves by translation[2], all else stays."""
        if self.attribute != abi.LAS_ELEVATION:
            return self
        t = np.float64(translation[2])
        return Style(self.attribute, float(np.float64(self.lo) + t), float(np.float64(self.hi) + t), self.lut)

    def record(self):
        """The SimlodLasStyle record (abi.las_style_dtype)."""
        r = np.zeros(1, dtype=abi.las_style_dtype)
        r["attribute"], r["lo"], r["hi"], r["lut"] = self.attribute, self.lo, self.hi, self.lut
        return r


def decode_records(records, bytes_per_point, fmt, scale, offset, style=None):
    """What simlod_decode_las_styled writes for these raw records, in numpy float64 (offset = header.offset + translation, as decode_offset forms
    it; an elevation window is in that frame: Style.in_frame).  style None: what simlod_decode_las writes.  ValueError where the call refuses."""
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, bytes_per_point)
    n = len(rec)
    field = lambda off, dt: np.ascontiguousarray(rec[:, off:off + int(dt[1])]).view("<" + dt).reshape(n)
    rgb_off = (RGB_OFFSET if style is None else RGB_OFFSET_ALL).get(fmt, 0)
    if not 12 <= bytes_per_point <= 255 or (style is not None and not 0 <= fmt <= 10) or (rgb_off and rgb_off + 6 > bytes_per_point):
        raise ValueError(f"format {fmt} in records of {bytes_per_point} bytes")
    out = np.zeros(n, dtype=abi.point_dtype)
    xyz = np.ascontiguousarray(rec[:, 0:12]).view("<i4").reshape(n, 3).astype(np.float64)
    pos = [xyz[:, k] * np.float64(scale[k]) + np.float64(offset[k]) for k in range(3)]           # one fp64 multiply, one fp64 add
    for k, name in enumerate("xyz"):
        out[name] = pos[k].astype(np.float32)
    color = np.full(n, 0xff000000, dtype=np.uint32)
    if style is None or style.attribute == abi.LAS_RGB:
        if rgb_off:
            c = np.ascontiguousarray(rec[:, rgb_off:rgb_off + 6]).view("<u2").reshape(n, 3).astype(np.uint32)
            c = np.where(c > 255, c // 256, c)
            color |= c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)
        out["color"] = color
        return out
    lo, hi = np.float64(style.lo), np.float64(style.hi)
    if not 0 <= style.attribute < abi.LAS_ATTRIBUTE_COUNT or not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"attribute {style.attribute} over [{lo}, {hi})")
    if style.attribute == abi.LAS_ELEVATION:
        v = pos[2]                                                 # the fp64 value z is rounded from
    else:
        off, kind, shift, mask = las_field(style.attribute, fmt)
        if off + int(kind[1]) > bytes_per_point:
            raise ValueError(f"the field ends beyond the record's {bytes_per_point} bytes")
        if kind == "f8":
            v = field(off, "f8")
        else:
            bits = (field(off, "u" + kind[1]).astype(np.int64) >> shift) & mask
            sign = (mask + 1) >> 1 if kind[0] == "i" else 0
            v = ((bits ^ sign) - sign).astype(np.float64)
            if kind == "i2":
                v = v * np.float64(0.006)                          # degrees per step of the 16-bit scan angle
    with np.errstate(all="ignore"):
        inv = np.float64(256.0) / (hi - lo)
        t = (v - lo) * inv                                         # fp64 subtract, then fp64 multiply
        idx = np.where(t >= 256.0, 255, np.where((t >= 0.0) & (t < 256.0), t, 0.0).astype(np.uint32))      # a NaN: 0
    out["color"] = color | (style.lut[idx] & np.uint32(0xffffff))
    return out


def write_las(path, records, fmt, scale, offset, mins, maxs, version=(1, 2), header_size=None, vlr_bytes=0, num_points=None):
    """Minimal LAS file: public header block (227 B for 1.2, 375 B for 1.4), `vlr_bytes` of filler, the point records
    (`num_points`: the count the header announces when the records are appended later)."""
    n, bpp = records.shape
    if num_points is not None:
        n = num_points
    major, minor = version
    hs = header_size if header_size is not None else (375 if minor >= 4 else 227)
    b = bytearray(hs)
    b[0:4] = b"LASF"
    b[24], b[25] = major, minor
    struct.pack_into("<H", b, 94, hs)
    struct.pack_into("<I", b, 96, hs + vlr_bytes)
    b[104] = fmt
    struct.pack_into("<H", b, 105, bpp)
    struct.pack_into("<I", b, 107, n if minor <= 3 else min(n, 0xffffffff))
    struct.pack_into("<3d", b, 131, *scale)
    struct.pack_into("<3d", b, 155, *offset)
    for k in range(3):
        struct.pack_into("<d", b, 179 + 16 * k, maxs[k])
        struct.pack_into("<d", b, 187 + 16 * k, mins[k])
    if minor >= 4:
        struct.pack_into("<Q", b, 247, n)
    with open(path, "wb") as f:
        f.write(bytes(b))
        f.write(bytes(vlr_bytes))
        f.write(records.tobytes())


def points_to_las(path, points, box_size, fmt=2, scale=0.001, world_min=(0.0, 0.0, 0.0), version=(1, 2), seed=0, chunk=4_000_000):
    """Synthetic LAS file whose decoded (translated) positions are close to `points`: X = round((x + world_min) / scale).
    Written `chunk` records at a time (a 350 M-point file is 9 GB; its records never exist in memory all at once)."""
    wm = np.asarray(world_min, dtype=np.float64)
    n = len(points)
    write_las(path, np.zeros((0, FORMAT_BYTES[fmt]), dtype=np.uint8), fmt, (scale,) * 3, (0.0, 0.0, 0.0), wm, wm + np.asarray(box_size, dtype=np.float64), version=version, num_points=n)
    with open(path, "ab") as f:
        for i in range(0, n, chunk):
            p = points[i:i + chunk]
            xyz = np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float64) + wm
            xyz_int = np.rint(xyz / scale).astype(np.int64).astype(np.int32)
            c = p["color"]
            rgb8 = np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], axis=1).astype(np.uint16)
            rgb16 = rgb8 * np.uint16(256) + rgb8                   # 16-bit colour as scanners write it; decodes back to rgb8
            f.write(las_records(xyz_int, rgb16, fmt, seed=seed + i // chunk).tobytes())
    return load_header(path)
