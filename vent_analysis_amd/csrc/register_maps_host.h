// register_maps_host.h -- the host side of the fine registration (register_maps.hip): the limits of a
// candidate count, the candidate list of one axis and the pick, in double; the spec is in
// include/vent_hip.h.  Standard headers only: tests/register_maps_check.cpp builds it with g++ alone under
// the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "resample_host.h"

#define RM_MAX_KR 17
#define RM_MAX_KC 17
#define RM_MAX_KZ 5

// count = (Kr, Kc, Kz) with 1 <= Kr, Kc <= 17 and 1 <= Kz <= 5
inline bool rm_count_in_limits(const int32_t *count) {
    return count && count[0] >= 1 && count[0] <= RM_MAX_KR && count[1] >= 1 && count[1] <= RM_MAX_KC &&
           count[2] >= 1 && count[2] <= RM_MAX_KZ;
}

// home inside its lists; null stands for the middle entries
inline bool rm_home_in_lists(const int32_t *count, const int32_t *home) {
    if (!home) return true;
    for (int a = 0; a < 3; ++a)
        if (home[a] < 0 || home[a] >= count[a]) return false;
    return true;
}

// The candidates of one axis around the base (s0, o0): factor f scales about the destination centre
// c = (n_dst - 1) / 2, then shift d (in destination voxels) moves.  Entry fi * ns + si is
// scale = s0 * f, offset = o0 + s0 * (c * (1 - f) + d), every operation a separately rounded double in
// that order.  False, with nothing written, for a null pointer, an empty list, n_dst outside 1..2^20 or a
// result outside the resampler's limits.
inline bool rm_axis_candidates(double s0, double o0, int64_t n_dst, const double *factors, int32_t nf,
                               const double *shifts, int32_t ns, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!factors || !shifts || !out || nf < 1 || ns < 1 || n_dst < 1 || n_dst > RS_MAX_DST) return false;
    const double c = ((double)n_dst - 1.0) / 2.0;
    for (int pass = 0; pass < 2; ++pass)   // (the checks first: a refusal writes nothing)
        for (int32_t fi = 0; fi < nf; ++fi)
            for (int32_t si = 0; si < ns; ++si) {
                const double f = factors[fi], d = shifts[si];
                const double scale = s0 * f;
                const double one_f = 1.0 - f;
                const double lever = c * one_f;
                const double moved = lever + d;
                const double in_src = s0 * moved;
                const double offset = o0 + in_src;
                if (pass == 0) {
                    if (!rs_map_in_limits(scale, offset)) return false;
                } else {
                    double *at = out + 2 * ((int64_t)fi * ns + si);
                    at[0] = scale;
                    at[1] = offset;
                }
            }
    return true;
}

// The best candidate (kr, kc, kz) of one study's scores [nc], index (kz Kr + kr) Kc + kc: the largest
// score; among equal scores the smallest |kr - hr| + |kc - hc| + |kz - hz|, then the lowest index.  A NaN
// never wins: with nothing but NaN the pick is home.  home null: the middle entry (K - 1) / 2 of each
// list.  False for a null pointer, a count outside its limits or home outside its list.
inline bool rm_pick(const double *score, const int32_t *count, const int32_t *home, int32_t *best) {
    if (!score || !best || !rm_count_in_limits(count) || !rm_home_in_lists(count, home)) return false;
    const int Kr = count[0], Kc = count[1], Kz = count[2];
    int32_t h[3];
    for (int a = 0; a < 3; ++a) h[a] = home ? home[a] : (count[a] - 1) / 2;
    int32_t at[3] = {h[0], h[1], h[2]};
    int l1 = -1;
    double top = 0.0;
    int64_t i = 0;
    for (int kz = 0; kz < Kz; ++kz)
        for (int kr = 0; kr < Kr; ++kr)
            for (int kc = 0; kc < Kc; ++kc, ++i) {
                const double v = score[i];
                if (std::isnan(v)) continue;
                const int d = std::abs(kr - h[0]) + std::abs(kc - h[1]) + std::abs(kz - h[2]);
                if (l1 < 0 || v > top || (v == top && d < l1)) {
                    top = v; l1 = d;
                    at[0] = kr; at[1] = kc; at[2] = kz;
                }
            }
    best[0] = at[0]; best[1] = at[1]; best[2] = at[2];
    return true;
}
