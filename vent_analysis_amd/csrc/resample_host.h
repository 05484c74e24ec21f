// resample_host.h -- the host side of the proton resampler (resample.hip): the tap table of one axis and
// the limits of a map, in double; the spec is in include/vent_hip.h.  Standard headers only:
// tests/resample_taps_check.cpp builds it with g++ alone under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

#define RS_TAPS 8            // VH_RESAMPLE_TAPS
#define RS_MAX_SRC 1024      // the largest source dimension
#define RS_MAX_DST (1 << 20) // the largest destination dimension a table is made for

// scale finite in [0.25, 4], offset finite with |offset| <= 2^20 (a NaN fails every comparison)
inline bool rs_map_in_limits(double scale, double offset) {
    return scale >= 0.25 && scale <= 4.0 && offset >= -1048576.0 && offset <= 1048576.0;
}

// The taps of every destination index of one axis.  first [n_dst], count [n_dst], weight [n_dst][8]:
// the in-range taps are source indices first .. first + count - 1 with weight[0 .. count - 1], the
// other slots 0.0f; first is 0 where count is 0.  False, with nothing written, for arguments outside
// the limits.
inline bool rs_axis_taps(int64_t n_src, int64_t n_dst, double scale, double offset, int32_t *first,
                         int32_t *count, float *weight) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!first || !count || !weight || n_src < 1 || n_src > RS_MAX_SRC || n_dst < 1 || n_dst > RS_MAX_DST ||
        !rs_map_in_limits(scale, offset))
        return false;
    const double w = scale > 1.0 ? scale : 1.0;
    for (int64_t i = 0; i < n_dst; ++i) {
        const double prod = scale * (double)i;
        const double u = prod + offset;
        // every j with t_j > 0 lies strictly inside (u - w, u + w): the integers from two below to two
        // above cover whatever the two roundings do
        const int64_t lo = (int64_t)std::floor(u - w) - 1, hi = (int64_t)std::ceil(u + w) + 1;
        double t[RS_TAPS];
        int64_t j0 = 0;
        int n = 0;
        double W = 0.0;
        for (int64_t j = lo; j <= hi; ++j) {
            const double d = std::fabs((double)j - u);
            const double q = d / w;
            const double tj = 1.0 - q;
            if (!(tj > 0.0)) continue;
            if (n == RS_TAPS) return false;   // (cannot happen: an open interval of length <= 8)
            if (n == 0) j0 = j;
            t[n++] = tj;
            W = W + tj;
        }
        float *wt = weight + RS_TAPS * i;
        for (int k = 0; k < RS_TAPS; ++k) wt[k] = 0.0f;
        int32_t f = 0, c = 0;
        for (int k = 0; k < n; ++k) {
            const int64_t j = j0 + k;
            if (j < 0 || j >= n_src) continue;   // dropped after the normalisation: zeros outside
            if (c == 0) f = (int32_t)j;
            wt[c++] = (float)(t[k] / W);
        }
        first[i] = f;
        count[i] = c;
    }
    return true;
}
