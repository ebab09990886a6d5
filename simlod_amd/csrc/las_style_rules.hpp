// las_style_rules.hpp — what simlod_decode_las_styled accepts and where an attribute lies in a record (include/simlod_hip.h, "styled decode";
// ASPRS LAS 1.4 R15, tables 7-17).  Plain host C++: the launcher in loader.hip and tests/host/las_style_check.cpp share it.
#pragma once
#include <cmath>
#include <stdint.h>

#include "simlod_hip.h"

namespace simlod {

// how the decode kernel forms v from the record
enum : uint32_t {
	LAS_KIND_RGB = 0,     // no v: the RGB triple at `offset` (0: the format has none, the point stays black)
	LAS_KIND_INT,         // the dword at `offset`: v = (double)sign_extend((dword >> shift) & mask) * mul
	LAS_KIND_F64,         // the double at `offset`
	LAS_KIND_Z,           // the fp64 z of the position
};

struct LasField {
	uint32_t kind, offset;
	uint32_t bytes;               // of the record from `offset` on that the field needs
	uint32_t shift, mask, sign;   // LAS_KIND_INT; sign: the field's sign bit after the shift (0: unsigned)
	double   mul;                 // LAS_KIND_INT: 1.0, or the 0.006 degrees of a 16-bit scan angle step
};

// RGB byte offset of every format that carries the triple (the reference's list, LasLoader.cpp:177-185, stops at 7); 0: none
inline uint32_t las_rgb_offset(uint32_t format) {
	switch (format) {
		case 2: return 20;
		case 3: case 5: return 28;
		case 7: case 8: case 10: return 30;
		default: return 0;
	}
}

// the field of `attribute` in a record of `format`; false: an unknown attribute or format, or an attribute the format lacks
inline bool las_field(uint32_t attribute, uint32_t format, LasField& f) {
	if (format > 10) return false;
	const bool ext = format >= 6;                                  // the 30-byte core of LAS 1.4
	auto integer = [&](uint32_t offset, uint32_t bytes, uint32_t shift, uint32_t mask, uint32_t sign, double mul) {
		f = LasField{LAS_KIND_INT, offset, bytes, shift, mask, sign, mul};
		return true;
	};
	switch (attribute) {
		case SIMLOD_LAS_RGB:               f = LasField{LAS_KIND_RGB, las_rgb_offset(format), 6, 0, 0, 0, 1.0}; return true;
		case SIMLOD_LAS_INTENSITY:         return integer(12, 2, 0, 0xffffu, 0, 1.0);
		case SIMLOD_LAS_RETURN_NUMBER:     return integer(14, 1, 0, ext ? 0xfu : 0x7u, 0, 1.0);
		case SIMLOD_LAS_NUMBER_OF_RETURNS: return integer(14, 1, ext ? 4 : 3, ext ? 0xfu : 0x7u, 0, 1.0);
		case SIMLOD_LAS_CLASSIFICATION:    return ext ? integer(16, 1, 0, 0xffu, 0, 1.0) : integer(15, 1, 0, 0x1fu, 0, 1.0);
		case SIMLOD_LAS_USER_DATA:         return integer(17, 1, 0, 0xffu, 0, 1.0);
		case SIMLOD_LAS_SCAN_ANGLE:        return ext ? integer(18, 2, 0, 0xffffu, 0x8000u, 0.006) : integer(16, 1, 0, 0xffu, 0x80u, 1.0);
		case SIMLOD_LAS_POINT_SOURCE_ID:   return integer(ext ? 20 : 18, 2, 0, 0xffffu, 0, 1.0);
		case SIMLOD_LAS_GPS_TIME:
			if (format == 0 || format == 2) return false;
			f = LasField{LAS_KIND_F64, ext ? 22u : 20u, 8, 0, 0, 0, 1.0};
			return true;
		case SIMLOD_LAS_ELEVATION:         f = LasField{LAS_KIND_Z, 8, 4, 0, 0, 0, 1.0}; return true;
		default: return false;
	}
}

// Everything of a styled call that can be judged without the device pointers: true, and the field, iff the call may go on.
inline bool las_style_acceptable(const SimlodLasStyle& s, uint32_t bytesPerPoint, uint32_t format, LasField& f) {
	if (s.reserved != 0 || !las_field(s.attribute, format, f)) return false;
	if (f.kind == LAS_KIND_RGB) return f.offset == 0 || f.offset + f.bytes <= bytesPerPoint;
	if (!std::isfinite(s.lo) || !std::isfinite(s.hi) || !(s.hi > s.lo)) return false;
	return f.offset + f.bytes <= bytesPerPoint;
}

}  // namespace simlod
