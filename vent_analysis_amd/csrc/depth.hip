// depth.hip -- the core-rind analysis of a resident batch (vh_batch_core_rind): per voxel of the mask
// the squared in-plane Euclidean distance D2 to the nearest clear pixel of its slice (the ring outside
// the slice is clear), as a saturated uint16 map, and per study the voxels and defect voxels of every
// depth band, the mask's size and its largest D2; the spec is in include/vent_hip.h.  Everything is an
// integer: the map and the counts are exact and do not depend on the order of the adds.
//
// The transform is separable.  g(r, c) is the distance from (r, c) to the nearest clear pixel of its
// own column (0 where the mask is clear, r + 1 and R - r at most: the ring), two run-length walks
// along the rows (k_depth_cols, into a scratch volume of the batch's shape).  Then D2(r, c) = min over
// dx of g(r, c + dx)^2 + dx^2, where a column outside the slice has g = 0 (k_depth_search).  The search
// walks dx = 1, 2, ... on both sides and stops as soon as dx^2 >= the best so far: no farther column
// can win, so the result is exact, and the walk is as long as the voxel is deep (the ring ends it at
// the latest).  The search has two forms (vh_core_rind_form): k_depth_rows stages the rows a workgroup
// searches in LDS; when a single row of g does not fit there, k_depth_search reads g through the
// caches.  Between them every shape the batch accepts is taken.
#include <algorithm>

#include "vh_internal.h"

#define DP_TPB 256
#define DP_BANDS 32                 // n_thr <= 31
#define DP_HEAD (2 * DP_BANDS + 2 + DP_BANDS / 2)   // the workgroup's LDS words: counts, max D2 (and one unused), thresholds
#define DP_COL 16                   // rows of a column walk whose loads are in flight together
#define DP_PER 8                    // voxels per thread whose own loads are in flight together
#define DP_SPAN 4096                // voxels a workgroup of k_depth_rows takes (whole rows; one row when it is longer)
#define DP_ROW_LDS (60 * 1024)      // bytes of g a workgroup of k_depth_rows may stage: no launch attribute needed

struct DpThr {                      // the thresholds, by value
    uint16_t t[DP_BANDS];
    int32_t n;
};

// the workgroup's counters and thresholds, in LDS
struct DpShared {
    uint32_t *cnt;                  // [DP_BANDS][2]: the band's voxels of M, and those with a defect
    uint32_t *mx;                   // [1] the largest D2
    uint16_t *thr;                  // [n_thr]
};

__device__ __forceinline__ DpShared dp_shared(uint32_t *head) {
    DpShared s;
    s.cnt = head;
    s.mx = head + 2 * DP_BANDS;     // (+ 1: unused)
    s.thr = reinterpret_cast<uint16_t *>(head + 2 * DP_BANDS + 2);
    return s;
}

__device__ __forceinline__ void dp_init(const DpShared &s, uint32_t *head, const DpThr &thr, int t) {
    for (int i = t; i < 2 * DP_BANDS + 2; i += DP_TPB) head[i] = 0u;
    for (int i = t; i < thr.n; i += DP_TPB) s.thr[i] = thr.t[i];
}

// D2 of a voxel whose column distance is g0 > 0: gp points at its g, the same row's columns are
// `stride` elements apart, it stands in column c of C.  Two steps of dx per round, their four loads in
// flight together and none behind a branch: a column outside the slice is read at the clamped
// offset and then counts as g = 0.  The second step is taken whether or not dx^2 >= best by then:
// every candidate is the squared distance to a clear pixel, so one more never lowers the minimum.
template <typename G>
__device__ __forceinline__ uint32_t dp_search(const G *gp, uint32_t g0, int stride, int c, int C) {
    uint32_t best = g0 * g0;
    const int left = c, right = C - 1 - c;   // columns on either side
    for (int dx = 1; (uint32_t)(dx * dx) < best; dx += 2) {
        uint32_t gv[4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            gv[2 * u] = gp[-min(dx + u, left) * stride];
            gv[2 * u + 1] = gp[min(dx + u, right) * stride];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t gl = dx + u <= left ? gv[2 * u] : 0u;
            const uint32_t gr = dx + u <= right ? gv[2 * u + 1] : 0u;
            const uint32_t gm = min(gl, gr);
            best = min(best, gm * gm + (uint32_t)((dx + u) * (dx + u)));
        }
    }
    return best;
}

// One column's g: src[r * stride] != 0 is the mask of row r, col[r * stride] receives g.  The downward
// run is stored saturated to G's range; it is only compared with 0 and with the upward run.  Down: the run
// length of set pixels ending at the row (the ring above row 0 is clear); up: the same from below, and
// the smaller of the two.  The rows go in groups of DP_COL whose loads
// are issued together and whose stores follow together: with one row per step every load would wait
// for the store in front of it (the compiler cannot tell that rows a runtime stride apart differ), a
// chain of 2 R memory latencies per pass.
template <typename G>
__device__ __forceinline__ void dp_walk_column(const uint8_t *__restrict__ src, G *__restrict__ col, int R,
                                               int64_t stride) {
    constexpr uint32_t G_MAX = (G)~(G)0;     // a downward run may pass it; g = min(down, up) does not (vh_depth_launch)
    uint32_t v[DP_COL];
    uint32_t run = 0u;
    int r = 0;
    for (; r + DP_COL <= R; r += DP_COL) {   // whole groups: no condition on a load or a store
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) v[u] = (uint32_t)src[(r + u) * stride];
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) {
            run = v[u] ? run + 1u : 0u;
            v[u] = min(run, G_MAX);
        }
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) col[(r + u) * stride] = (G)v[u];
    }
    for (; r < R; ++r) {                     // the last R % DP_COL rows
        run = src[r * stride] ? run + 1u : 0u;
        col[r * stride] = (G)min(run, G_MAX);
    }
    run = 0u;                                // the ring below row R - 1 is clear too
    r = R;
    for (; r - DP_COL >= 0; r -= DP_COL) {
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) v[u] = (uint32_t)col[(r - 1 - u) * stride];
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) {
            run = v[u] ? run + 1u : 0u;
            v[u] = min(v[u], run);
        }
#pragma unroll
        for (int u = 0; u < DP_COL; ++u) col[(r - 1 - u) * stride] = (G)v[u];
    }
    for (--r; r >= 0; --r) {
        const uint32_t down = col[r * stride];
        run = down ? run + 1u : 0u;
        col[r * stride] = (G)min(down, run);
    }
}

// A thread's voxels of one band in a row cost one LDS atomic pair, not one each: neighbours along a
// thread's walk mostly share the band.
struct DpRun {
    int band = 0;
    uint32_t nm = 0u, nd = 0u;
};

__device__ __forceinline__ void dp_flush(DpRun &run, const DpShared &s) {
    if (run.nm) atomicAdd(&s.cnt[2 * run.band], run.nm);
    if (run.nd) atomicAdd(&s.cnt[2 * run.band + 1], run.nd);
    run.nm = run.nd = 0u;
}

// a voxel of M with squared distance d2 (saturated: d2s): the number of thresholds <= d2s is its band
__device__ __forceinline__ void dp_count(DpRun &run, const DpShared &s, int n_thr, uint32_t d2s, bool def) {
    int lo = 0, hi = n_thr;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)s.thr[mid] <= d2s) lo = mid + 1; else hi = mid;
    }
    if (lo != run.band) {
        dp_flush(run, s);
        run.band = lo;
    }
    ++run.nm;
    run.nd += def ? 1u : 0u;
}

// the workgroup's nonzero counters to the study's rows: counts [n_thr + 1][2], stats [2] = n_mask, max D2
__device__ __forceinline__ void dp_publish(const DpShared &s, int n_thr, int t, unsigned long long *counts,
                                           unsigned long long *stats) {
    if (t < 2 * (n_thr + 1) && s.cnt[t]) atomicAdd(&counts[t], (unsigned long long)s.cnt[t]);
    if (t == 64) {
        unsigned long long n = 0ull;
        for (int i = 0; i <= n_thr; ++i) n += s.cnt[2 * i];
        if (n) atomicAdd(&stats[0], n);
    }
    if (t == 65 && *s.mx) atomicMax(&stats[1], (unsigned long long)*s.mx);
}

// k_depth_cols, grid (column-slice pairs / DP_TPB, nb): thread j of the C Z pairs walks its column down
// and up; a wave reads and writes 64 consecutive elements of every row.
template <typename G>
__global__ void __launch_bounds__(DP_TPB) k_depth_cols(const uint8_t *__restrict__ mask, G *__restrict__ g, int64_t V,
                                                       int R, int64_t CZ) {
    const int64_t j = (int64_t)blockIdx.x * DP_TPB + threadIdx.x;
    if (j >= CZ) return;
    dp_walk_column(mask + (int64_t)blockIdx.y * V + j, g + (int64_t)blockIdx.y * V + j, R, CZ);
}

// k_depth_search, grid (voxels / (DP_TPB DP_PER), nb): a workgroup takes a run of voxels, thread t
// its elements t, t + DP_TPB, ...; the search reads g through the caches.
template <typename G>
__global__ void __launch_bounds__(DP_TPB) k_depth_search(const G *__restrict__ g, const uint8_t *__restrict__ defect,
                                                         uint16_t *__restrict__ map, int64_t V, int C, int Z, DpThr thr,
                                                         unsigned long long *counts, unsigned long long *stats) {
    __shared__ uint32_t s_head[DP_HEAD];
    const DpShared sh = dp_shared(s_head);
    const int t = threadIdx.x;
    const int64_t sb = blockIdx.y;
    const G *gs = g + sb * V;
    const uint8_t *ds = defect ? defect + sb * V : nullptr;
    uint16_t *out = map + sb * V;
    dp_init(sh, s_head, thr, t);
    __syncthreads();

    DpRun run;
    uint32_t mx = 0u;
    const int64_t e0 = (int64_t)blockIdx.x * (DP_TPB * DP_PER) + t;
    uint32_t gv[DP_PER], dv[DP_PER];   // the thread's own g and defect bytes first, in flight together
    const uint8_t *dl = ds ? ds : reinterpret_cast<const uint8_t *>(gs);   // (no defect map: loads that are not used)
#pragma unroll
    for (int k = 0; k < DP_PER; ++k) {
        const int64_t e = min(e0 + (int64_t)k * DP_TPB, V - 1);   // (clamped: a load without a branch)
        gv[k] = gs[e];
        dv[k] = dl[e];
    }
#pragma unroll
    for (int k = 0; k < DP_PER; ++k) {
        const int64_t e = e0 + (int64_t)k * DP_TPB;
        if (e >= V) break;
        uint32_t d2 = 0u;
        if (gv[k]) {
            const int c = (int)(((uint32_t)e / (uint32_t)Z) % (uint32_t)C);   // V < 2^31 (check_dims)
            d2 = dp_search(gs + e, gv[k], Z, c, C);
            mx = max(mx, d2);
            dp_count(run, sh, thr.n, min(d2, 65535u), ds && dv[k] != 0u);
        }
        out[e] = (uint16_t)min(d2, 65535u);
    }
    dp_flush(run, sh);
    if (mx) atomicMax(sh.mx, mx);
    __syncthreads();
    dp_publish(sh, thr.n, t, counts + sb * 2 * (thr.n + 1), stats + sb * 2);
}

// k_depth_rows, grid (rows / nr, nb): the search with its reads in LDS.  A workgroup takes nr whole
// rows, one contiguous run of g, and stages it; a search never leaves its voxel's row, so nothing else
// is read, and a round of the search costs an LDS latency, not a cache's.  Thread t takes elements t,
// t + DP_TPB, ... of the run, DP_PER at a time with their defect bytes in flight together.
template <typename G>
__global__ void __launch_bounds__(DP_TPB) k_depth_rows(const G *__restrict__ g, const uint8_t *__restrict__ defect,
                                                       uint16_t *__restrict__ map, int64_t V, int R, int C, int Z, int nr,
                                                       DpThr thr, unsigned long long *counts,
                                                       unsigned long long *stats) {
    extern __shared__ __align__(16) uint32_t s_dp[];
    const DpShared sh = dp_shared(s_dp);
    G *s_g = reinterpret_cast<G *>(s_dp + DP_HEAD);
    const int t = threadIdx.x;
    const int64_t sb = blockIdx.y;
    const int r0 = (int)blockIdx.x * nr;
    const int n = min(nr, R - r0) * C * Z;   // <= DP_ROW_LDS elements (dp_rows)
    const int64_t base = sb * V + (int64_t)r0 * C * Z;
    const G *gs = g + base;
    const uint8_t *ds = defect ? defect + base : nullptr;
    uint16_t *out = map + base;
    dp_init(sh, s_dp, thr, t);
#pragma unroll 4
    for (int i = t; i < n; i += DP_TPB) s_g[i] = gs[i];
    __syncthreads();

    DpRun run;
    uint32_t mx = 0u;
    const uint8_t *dl = ds ? ds : reinterpret_cast<const uint8_t *>(gs);   // (no defect map: loads that are not used)
    for (int e0 = t; e0 < n; e0 += DP_PER * DP_TPB) {
        uint32_t dv[DP_PER];
#pragma unroll
        for (int k = 0; k < DP_PER; ++k) dv[k] = dl[min(e0 + k * DP_TPB, n - 1)];   // (clamped: a load without a branch)
#pragma unroll
        for (int k = 0; k < DP_PER; ++k) {
            const int e = e0 + k * DP_TPB;
            if (e >= n) break;
            const uint32_t g0 = s_g[e];
            uint32_t d2 = 0u;
            if (g0) {
                const int c = (int)(((uint32_t)e / (uint32_t)Z) % (uint32_t)C);
                d2 = dp_search(s_g + e, g0, Z, c, C);
                mx = max(mx, d2);
                dp_count(run, sh, thr.n, min(d2, 65535u), ds && dv[k] != 0u);
            }
            out[e] = (uint16_t)min(d2, 65535u);
        }
    }
    dp_flush(run, sh);
    if (mx) atomicMax(sh.mx, mx);
    __syncthreads();
    dp_publish(sh, thr.n, t, counts + sb * 2 * (thr.n + 1), stats + sb * 2);
}

// Rows per workgroup of k_depth_rows for rows of CZ elements of gsize bytes: about DP_SPAN voxels, at
// least one row; 0 when a row does not fit DP_ROW_LDS, and k_depth_search takes the shape.
static int dp_rows(int64_t CZ, int64_t gsize) {
    if (CZ * gsize > DP_ROW_LDS) return 0;
    return (int)std::max<int64_t>(1, DP_SPAN / CZ);
}

static int64_t dp_gsize(int64_t R) { return R <= 510 ? 1 : 2; }   // g <= min(r + 1, R - r) <= 255 when R <= 510

int vh_depth_form(int64_t R, int64_t C, int64_t Z) { return dp_rows(C * Z, dp_gsize(R)) ? 0 : 1; }

bool vh_depth_takes(const vh_batch *b) { return b->nb <= 65535; }   // grid y; x is far below 2^31 (check_dims)

template <typename G>
static void dp_launch(vh_batch *b, const uint8_t *defect, const DpThr &th, G *d_g, uint16_t *map,
                      unsigned long long *d_counts, unsigned long long *d_stats) {
    hipStream_t st = b->stream;
    const dim3 gc((unsigned)((b->CZ + DP_TPB - 1) / DP_TPB), (unsigned)b->nb, 1);
    k_depth_cols<G><<<gc, DP_TPB, 0, st>>>(b->d_mask, d_g, b->V, (int)b->R, b->CZ);
    VH_CHECK_LAUNCH();
    if (const int nr = dp_rows(b->CZ, sizeof(G))) {
        const size_t lds = 4 * DP_HEAD + sizeof(G) * (size_t)std::min<int64_t>(nr, b->R) * b->CZ;
        const dim3 gr((unsigned)((b->R + nr - 1) / nr), (unsigned)b->nb, 1);
        k_depth_rows<G><<<gr, DP_TPB, lds, st>>>(d_g, defect, map, b->V, (int)b->R, (int)b->C, (int)b->Z, nr, th,
                                                 d_counts, d_stats);
    } else {
        const int64_t per = DP_TPB * DP_PER;
        const dim3 gs((unsigned)((b->V + per - 1) / per), (unsigned)b->nb, 1);
        k_depth_search<G><<<gs, DP_TPB, 0, st>>>(d_g, defect, map, b->V, (int)b->C, (int)b->Z, th, d_counts, d_stats);
    }
    VH_CHECK_LAUNCH();
}

void vh_depth_launch(vh_batch *b, const uint8_t *defect, const uint16_t *thr, int n_thr, uint16_t *d_g, uint16_t *map,
                     unsigned long long *d_counts, unsigned long long *d_stats) {
    hipStream_t st = b->stream;
    DpThr th{};
    th.n = n_thr;
    std::copy(thr, thr + n_thr, th.t);
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t)b->nb * 2 * (n_thr + 1), st));
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * (size_t)b->nb * 2, st));
    // the algorithmic bytes: the mask and the defect read, the map written (g's round trips are the
    // method's, not the problem's)
    ScopedKTimer tm(b, "depth_b", (defect ? 4.0 : 3.0) * (double)b->nb * (double)b->V);
    // a byte per voxel of scratch traffic instead of two where g fits one
    if (dp_gsize(b->R) == 1)
        dp_launch(b, defect, th, reinterpret_cast<uint8_t *>(d_g), map, d_counts, d_stats);
    else
        dp_launch(b, defect, th, d_g, map, d_counts, d_stats);
}
