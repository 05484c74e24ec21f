// zones_host.h -- the zone rule of the regional analysis (zones.hip): the bounds of a mask profile, the
// parts of an axis, the lateral split and the zone of a voxel; the spec is in include/vent_hip.h.  The
// kernels and the two host functions (vh_zone_parts, vh_zone_split) call the same functions, over
// uint32 profiles on the device and int64 ones on the host.  Every value is an integer.  Standard
// headers only: tests/zones_state_check.cpp builds it with g++ alone under the sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ZN_HD __host__ __device__
#else
#define ZN_HD
#endif

#define ZN_EXTENT 0          // VH_ZONE_EXTENT
#define ZN_COUNT 1           // VH_ZONE_COUNT
#define ZN_MAX_PARTS 32      // the most parts of an axis, and the most zones

// lo / hi: the first / last index with P > 0 (0 / -1 for an all-zero profile), total: the sum of P
template <typename P>
ZN_HD inline void zn_bounds(const P *prof, int64_t n, int32_t &lo, int32_t &hi, int64_t &total) {
    lo = 0;
    hi = -1;
    total = 0;
    for (int64_t i = 0; i < n; ++i)
        if (prof[i] > 0) {
            if (hi < 0) lo = (int32_t)i;
            hi = (int32_t)i;
            total += (int64_t)prof[i];
        }
}

// by extent: clamp(floor((i - lo) p / w), 0, p - 1); 0 for an empty axis (w <= 0)
ZN_HD inline int32_t zn_part_extent(int64_t i, int32_t lo, int32_t w, int32_t p) {
    if (w <= 0 || i <= lo) return 0;   // (at and below lo the floored quotient is <= 0)
    const int64_t q = ((i - lo) * p) / w;
    return q > p - 1 ? p - 1 : (int32_t)q;
}

// by count: min(p - 1, cum p / total) with cum the voxels of the planes before this one; 0 for total 0
ZN_HD inline int32_t zn_part_count(int64_t cum, int64_t total, int32_t p) {
    if (total <= 0) return 0;
    const int64_t q = (cum * p) / total;
    return q > p - 1 ? p - 1 : (int32_t)q;
}

// the parts of every index of one axis: part [n]
template <typename P, typename T>
ZN_HD inline void zn_axis_parts(const P *prof, int64_t n, int32_t p, int by, int32_t lo, int32_t hi, int64_t total,
                                T *part) {
    if (by == ZN_EXTENT) {
        for (int64_t i = 0; i < n; ++i) part[i] = (T)zn_part_extent(i, lo, hi - lo + 1, p);
    } else {
        int64_t cum = 0;
        for (int64_t i = 0; i < n; ++i) {
            part[i] = (T)zn_part_count(cum, total, p);
            cum += prof[i] > 0 ? (int64_t)prof[i] : 0;
        }
    }
}

// the lateral split: the column of the smallest P among lo + w / 4 .. hi - w / 4, the smallest such
// column on a tie; 0 for an empty axis
template <typename P>
ZN_HD inline int32_t zn_split(const P *prof, int32_t lo, int32_t hi) {
    if (hi < lo) return 0;
    const int32_t q = (hi - lo + 1) / 4;
    int32_t s = lo + q;
    for (int32_t c = s + 1; c <= hi - q; ++c)
        if (prof[c] < prof[s]) s = c;
    return s;
}

// the zone of an on voxel from its three part indices (col: the side with a lateral split)
ZN_HD inline int32_t zn_zone(int32_t part_r, int32_t col, int32_t part_z, int32_t nc, int32_t pz) {
    return 1 + (part_r * nc + col) * pz + part_z;
}
