"""The styled LAS decode (include/simlod_hip.h, "styled decode") stated a second time, one record at a time with struct.unpack_from, straight from
the field table of ASPRS LAS 1.4 R15 (tables 7-17).  Nothing here comes from simlod_amd.lasio: lasio.decode_records has to equal this byte for byte."""
import struct

import numpy as np

(RGB, INTENSITY, CLASSIFICATION, RETURN_NUMBER, NUMBER_OF_RETURNS, USER_DATA, POINT_SOURCE_ID, SCAN_ANGLE, GPS_TIME, ELEVATION) = range(10)
NAMES = ["rgb", "intensity", "classification", "return_number", "number_of_returns", "user_data", "point_source_id", "scan_angle", "gps_time", "elevation"]
RGB_AT = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}
HAS_GPS_TIME = (1, 3, 4, 5, 6, 7, 8, 9, 10)
MIN_BYTES = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}


def has(attribute, fmt):
    return attribute != GPS_TIME or fmt in HAS_GPS_TIME


def value(rec, at, fmt, attribute, z64):
    """v of the colour rule for the record that starts at byte `at`."""
    old = fmt <= 5
    if attribute == INTENSITY:
        return float(struct.unpack_from("<H", rec, at + 12)[0])
    if attribute == RETURN_NUMBER:
        return float(rec[at + 14] & (0x07 if old else 0x0f))
    if attribute == NUMBER_OF_RETURNS:
        return float((rec[at + 14] >> 3) & 0x07 if old else rec[at + 14] >> 4)
    if attribute == CLASSIFICATION:
        return float(rec[at + 15] & 0x1f if old else rec[at + 16])
    if attribute == USER_DATA:
        return float(rec[at + 17])
    if attribute == SCAN_ANGLE:
        return float(struct.unpack_from("<b", rec, at + 16)[0]) if old else float(struct.unpack_from("<h", rec, at + 18)[0]) * 0.006
    if attribute == POINT_SOURCE_ID:
        return float(struct.unpack_from("<H", rec, at + (18 if old else 20))[0])
    if attribute == GPS_TIME:
        assert fmt in HAS_GPS_TIME
        return struct.unpack_from("<d", rec, at + (20 if old else 22))[0]
    assert attribute == ELEVATION
    return z64


def decode(records, bytes_per_point, fmt, scale, offset, attribute, lo, hi, lut):
    """-> (x, y, z as float32 arrays, colour words): the styled decode of `records` (bytes)."""
    rec = bytes(np.ascontiguousarray(records, dtype=np.uint8).reshape(-1))
    n = len(rec) // bytes_per_point
    xyz = np.zeros((n, 3), dtype=np.float32)
    colour = np.zeros(n, dtype=np.uint32)
    inv = None if attribute == RGB else 256.0 / (float(hi) - float(lo))
    for i in range(n):
        at = i * bytes_per_point
        X, Y, Z = struct.unpack_from("<3i", rec, at)
        p = (float(X) * float(scale[0]) + float(offset[0]), float(Y) * float(scale[1]) + float(offset[1]), float(Z) * float(scale[2]) + float(offset[2]))
        xyz[i] = p                                            # (rounds to nearest fp32)
        if attribute == RGB:
            c = 0
            if fmt in RGB_AT:
                ch = [v // 256 if v > 255 else v for v in struct.unpack_from("<3H", rec, at + RGB_AT[fmt])]
                c = ch[0] | (ch[1] << 8) | (ch[2] << 16)
        else:
            v = value(rec, at, fmt, attribute, p[2])
            t = (v - float(lo)) * inv
            idx = (int(t) if t < 256.0 else 255) if t >= 0.0 else 0
            c = int(lut[idx]) & 0xffffff
        colour[i] = 0xff000000 | c
    return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), colour
