// ci.hip -- cluster-index map on gfx950 (CI.calculate_CI, CI.py:107-145, and the 95th-percentile
// tail of Vent_Analysis.calculate_CI, Vent_Analysis.py:265-271).
//
// One wave per defect voxel (k_ci_walk): the wave's lanes test consecutive rows of the sphere table
// against the volume's defect bitmap and stop at the first shell boundary b with 2*hits < b
// (C = hits/b < 0.5, CI.py:97), recording the shell.
// Semantics restated in oracle/ci_oracle.c: the bitmap is indexed by the
// Fortran-order linear index L = (i+dx) + (j+dy) s0 + (k+dz) s0 s1 (px2vec, CI.py:65-68), so
// out-of-range rows/cols alias into neighbouring columns/slices and only 0 <= L < N is required;
// table rows whose linear offset repeats an earlier row never count (np.intersect1d uniques).
#include <algorithm>
#include <climits>

#include "vh_internal.h"

#define CI_SENTINEL INT32_MIN

// VH_DEBUG_BOUNDS builds (make DEBUG_BOUNDS=1 -> libventhip_dbg.so): every index the CI kernels
// derive from data (defect list slots, table rows, shells, bitmap words) is checked against its
// buffer's extent before the access; a violation skips the access and records (site, index, extent)
// in g_ci_dbg, which ci_debug_check() reads after the call's stream sync and raises as VH_ERR_HIP.
// Release builds compile the checks away (CI_OK(c, ...) == c is never evaluated as a guard).
#ifdef VH_DEBUG_BOUNDS
static __device__ unsigned long long g_ci_dbg[4];
__device__ __forceinline__ bool ci_ok(bool c, int site, int64_t idx, int64_t ext) {
    if (!c && atomicCAS(&g_ci_dbg[0], 0ull, (unsigned long long)site) == 0ull) {
        atomicExch(&g_ci_dbg[1], (unsigned long long)idx);
        atomicExch(&g_ci_dbg[2], (unsigned long long)ext);
    }
    return c;
}
#define CI_OK(c, site, idx, ext) ci_ok((c), (site), (int64_t)(idx), (int64_t)(ext))
#else
#define CI_OK(c, site, idx, ext) true
#endif

__global__ void k_ci_bitmap(const uint8_t *__restrict__ defect, int64_t s0, int64_t s1,
                            int64_t s2, int64_t V, int64_t words, uint32_t *bits,
                            int32_t *list, unsigned long long *count, int16_t *shell16) {
    const int64_t b = blockIdx.y;
    __shared__ unsigned long long s_cnt, s_base;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool d = false;
    unsigned long long my = 0;
    if (v < V) {
        d = defect[b * V + v] != 0;
        if (d) {
            const int64_t i = v / (s1 * s2), j = (v / s2) % s1, k = v % s2;
            const int64_t L = i + j * s0 + k * s0 * s1;
            if (CI_OK((L >> 5) < words, 1, L, words))
                atomicOr(&bits[b * words + (L >> 5)], 1u << (L & 31));
            my = atomicAdd(&s_cnt, 1ull);
        } else if (shell16) {
            shell16[b * V + v] = -1;   // vh_batch_ci's map: the walk writes the defect voxels, so no memset
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(&count[b], s_cnt) : 0ull;
    __syncthreads();
    if (d && CI_OK((int64_t)(s_base + my) < V, 2, s_base + my, V)) list[b * V + (int64_t)(s_base + my)] = (int32_t)v;
}

// The walk of one defect voxel by one wave (shared by k_ci_walk and k_ci_walk_b): the table as a
// workgroup sees it -- the first lrows offsets / lnbs boundaries in LDS, the rest in L2 -- the
// volume's Fortran-order bitmap bm (LDS or L2) and the voxel's px2vec index base.  Returns the shell
// at which the walk stops, -1 when it reaches the table's last radius.  Wave-uniform.
#define CIW_U 4
struct CiTab {
    const int32_t *offL, *bounds;     // the whole table (L2)
    const int32_t *s_off, *s_bnd;     // its head (LDS)
    int64_t rows, nbs;
    int lrows, lnbs;
};
__device__ __forceinline__ int32_t ci_walk_one(const CiTab &T, const uint32_t *bm, int64_t words,
                                               int64_t base, int64_t N, int lane) {
    const int64_t rows = T.rows, nbs = T.nbs;
    auto off_at = [&](int64_t r) {
        if (!CI_OK(r >= 0 && r < rows, 4, r, rows)) return (int32_t)CI_SENTINEL;
        return r < T.lrows ? T.s_off[r] : T.offL[r];
    };
    auto bnd_at = [&](int64_t q) {
        if (!CI_OK(q >= 0 && q < nbs, 5, q, nbs)) return (int64_t)INT64_MAX;
        return q < T.lnbs ? (int64_t)T.s_bnd[q] : (int64_t)T.bounds[q];
    };
    int64_t hits = 0, q = 0, row = 0;
    int32_t qstop = -1;
    while (q < nbs && row < rows) {
        uint64_t bal[CIW_U];
        int32_t off[CIW_U];
#pragma unroll
        for (int u = 0; u < CIW_U; ++u) {
            const int64_t r = row + 64 * u + lane;
            off[u] = r < rows ? off_at(r) : CI_SENTINEL;
        }
#pragma unroll
        for (int u = 0; u < CIW_U; ++u) {
            const int64_t L = base + off[u];
            const bool hit = off[u] != CI_SENTINEL && L >= 0 && L < N && CI_OK((L >> 5) < words, 7, L, words) &&
                             ((bm[L >> 5] >> (L & 31)) & 1u);
            bal[u] = __ballot(hit);
        }
        const int64_t rend = row + 64 * CIW_U;
        // boundaries in (row, rend], 64 per pass, in order
        bool stopped = false;
        for (;;) {
            const int64_t bq = q + lane < nbs ? bnd_at(q + lane) : INT64_MAX;
            const bool inc = bq <= rend;
            bool stop = false;
            if (inc) {
                int pos = (int)(bq - 1 - row);   // 0 .. 64 CIW_U - 1
                if (!CI_OK(pos >= 0 && pos < 64 * CIW_U, 8, pos, 64 * CIW_U)) pos = 0;
                const int u = pos >> 6, pb = pos & 63;
                int64_t c = hits;
#pragma unroll
                for (int uu = 0; uu < CIW_U; ++uu)
                    c += uu < u ? __popcll(bal[uu]) : uu == u ? __popcll(bal[uu] & (pb == 63 ? ~0ull : ((2ull << pb) - 1ull))) : 0;
                stop = 2 * c < bq;
            }
            const uint64_t sb = __ballot(stop);
            if (sb) {
                qstop = (int32_t)(q + __builtin_ctzll(sb));
                stopped = true;
                break;
            }
            const int ninc = __popcll(__ballot(inc));
            q += ninc;
            if (ninc < 64 || q >= nbs) break;
        }
        if (stopped) break;
#pragma unroll
        for (int u = 0; u < CIW_U; ++u) hits += __popcll(bal[u]);
        row = rend;
    }
    return qstop;
}

// One WAVE per defect voxel: the wave probes CIW_U x 64 consecutive table rows per step (lane l
// tests rows r0 + 64 u + l, u < CIW_U: the CIW_U loads are independent, so one step pays one memory
// latency for 256 rows), the step's hits are CIW_U ballots, and the shell boundaries that fall in
// the step are tested in parallel, 64 at a time (lane i takes the i-th boundary: cumulative hits up
// to row b - 1 are the hits before the step plus popcounts of the ballots below b's); the first
// boundary with 2 hits < b stops the walk.  Every probe of the lane-per-voxel form is made (same rows,
// same order of boundaries; rows past the stop in the last step are probed and ignored).  LDS holds
// the Fortran-order defect bitmap (48 KiB at 128x128x24) and the first CIW_ROWS rows of linear
// offsets and CIW_NBS boundaries (every walk shorter than r ~ 23 at [1.5, 1.5, 10] stays in LDS);
// later rows come from L2.  A block takes voxels blockIdx.x, blockIdx.x + gridDim.x, ... (16 waves
// each) and exits before staging anything when the volume has fewer defect voxels than its first.
#define CIW_TPB 1024
#define CIW_ROWS 8192
#define CIW_NBS 1024
#define CIW_LDS_MAX (160 * 1024)
__global__ void __launch_bounds__(CIW_TPB) k_ci_walk(const uint32_t *__restrict__ bits,
                                                    const int32_t *__restrict__ list,
                                                    const unsigned long long *count,
                                                    const int32_t *__restrict__ offL, int64_t rows,
                                                    const int32_t *__restrict__ bounds, int64_t nbs,
                                                    int64_t s0, int64_t s1, int64_t s2, int64_t V,
                                                    int64_t words, int stage_bits, int32_t *shell_of,
                                                    int16_t *shell16, uint32_t *hist, int32_t *status) {
    extern __shared__ uint32_t s_lds[];
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)count[b];
    constexpr int W = CIW_TPB / 64;
    if (!CI_OK(n <= V, 3, n, V)) return;
    if ((int64_t)blockIdx.x * W >= n) return;   // block-uniform exit, before any staging
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // LDS: offsets [CIW_ROWS], boundaries [CIW_NBS], then the bitmap (stage_bits)
    int32_t *s_off = reinterpret_cast<int32_t *>(s_lds), *s_bnd = s_off + CIW_ROWS;
    const int lrows = (int)(rows < CIW_ROWS ? rows : CIW_ROWS), lnbs = (int)(nbs < CIW_NBS ? nbs : CIW_NBS);
    for (int i = threadIdx.x; i < lrows; i += CIW_TPB) s_off[i] = offL[i];
    for (int i = threadIdx.x; i < lnbs; i += CIW_TPB) s_bnd[i] = bounds[i];
    const uint32_t *bm = bits + b * words;
    if (stage_bits) {
        uint32_t *s_bits = reinterpret_cast<uint32_t *>(s_bnd + CIW_NBS);
        for (int64_t i = threadIdx.x; i < words; i += CIW_TPB) s_bits[i] = bm[i];
        bm = s_bits;
    }
    __syncthreads();
    const CiTab T{offL, bounds, s_off, s_bnd, rows, nbs, lrows, lnbs};
    const int64_t N = s0 * s1 * s2;
    for (int64_t idx = (int64_t)blockIdx.x * W + w; idx < n; idx += (int64_t)gridDim.x * W) {
        const int32_t v = list[b * V + idx];
        if (!CI_OK(v >= 0 && v < V, 6, v, V)) continue;
        const int64_t i = v / (s1 * s2), j = (v / s2) % s1, k = v % s2;
        const int64_t base = i + j * s0 + k * s0 * s1;   // px2vec (Fortran order, CI.py:65-68)
        const int32_t qstop = ci_walk_one(T, bm, words, base, N, lane);
        if (lane == 0) {
            if (shell16) shell16[b * V + v] = (int16_t)qstop;   // vh_batch_ci (nbs <= 32767)
            else shell_of[b * V + v] = qstop;
            if (qstop >= 0 && CI_OK(qstop < nbs, 9, qstop, nbs)) atomicAdd(&hist[b * nbs + qstop], 1u);
            else atomicExch(&status[b], 1);
        }
    }
}

// The batch form (vh_batch_ci, VH_CI_FORM=2), grid (G, nb): a study's G workgroups stage once --
// the table's head (hrows offsets, CIB_NBS boundaries; the rest comes from L2 as in k_ci_walk), a
// shell histogram when nbs fits (lds_hist) and the study's bitmap when that fits too (stage_bits) --
// and their waves then take defect voxels from the study's list until it is empty.  A wave's first
// slot is its own (workgroup x, wave w: slot 16 x + w, no atomic); further slots come in runs of
// CIB_CHUNK from the study's counter, which counts from slot 16 G: walks last from 1 step to over
// 100, so a fixed stride would leave waves idle behind the longest.  A wave asks for its next run
// before it walks the current one, and a study of at most 16 G defect voxels issues no atomic at all.
// The counters are device-scope atomics, which one 128-byte line serves one after the other
// whatever the address in it: with the studies' counters packed 32 to a line the 256-study bench
// batch took 5.6 - 16.6 ms (more workgroups: slower) against k_ci_walk's 4.4, so each counter has
// 256 bytes to itself, and G is capped at CIB_G_MAX: more than ~512 waves on one counter wait for
// each other longer than they walk (DESIGN 4.4 has the sweep).
// The histogram is flushed once per workgroup, non-zero bins only, with vector atomics.  A plain
// launch: no workgroup waits for another, so it is safe beside cooperative N4 grids in flight.
// LDS: offsets, boundaries, histogram, bitmap.
#define CIB_ROWS 8192       // resident table rows by default (VH_CI_B_ROWS overrides)
#define CIB_NBS 1024
#define CIB_HIST_MAX 8192   // shells counted in LDS (32 KiB)
#ifndef CIB_CHUNK
#define CIB_CHUNK 2         // slots per claim (1 and 2 measured alike, 4 and up slower: DESIGN 4.4)
#endif
#define CIB_NEXT_STRIDE 64  // uint32 between two studies' counters (256 bytes)
#define CIB_WG_PER_CU 16    // workgroups per CU over the whole batch (VH_CI_B_G sets G itself)
#define CIB_G_MAX 32        // ... but at most this many per study (512 waves on the study's counter)
#define CIB_AUTO_MIN_NB 16  // auto: the batch form from this many studies up
__global__ void __launch_bounds__(CIW_TPB) k_ci_walk_b(const uint32_t *__restrict__ bits,
                                                      const int32_t *__restrict__ list,
                                                      const unsigned long long *count, uint32_t *next,
                                                      const int32_t *__restrict__ offL, int64_t rows,
                                                      const int32_t *__restrict__ bounds, int64_t nbs,
                                                      int64_t s0, int64_t s1, int64_t s2, int64_t V,
                                                      int64_t words, int hrows, int lds_hist, int stage_bits,
                                                      int16_t *shell16, uint32_t *hist, int32_t *status) {
    extern __shared__ uint32_t s_lds[];
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)count[b];
    constexpr int W = CIW_TPB / 64;
    if (!CI_OK(n <= V, 12, n, V)) return;
    if ((int64_t)blockIdx.x * W >= n) return;   // block-uniform exit, before any staging (empty studies too)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t *s_off = reinterpret_cast<int32_t *>(s_lds), *s_bnd = s_off + hrows;
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_bnd + CIB_NBS);
    const int lrows = (int)(rows < hrows ? rows : hrows), lnbs = (int)(nbs < CIB_NBS ? nbs : CIB_NBS);
    for (int i = threadIdx.x; i < lrows; i += CIW_TPB) s_off[i] = offL[i];
    for (int i = threadIdx.x; i < lnbs; i += CIW_TPB) s_bnd[i] = bounds[i];
    if (lds_hist)
        for (int i = threadIdx.x; i < (int)nbs; i += CIW_TPB) s_hist[i] = 0u;
    const uint32_t *bm = bits + b * words;
    if (stage_bits) {
        uint32_t *s_bits = s_hist + (lds_hist ? nbs : 0);
        for (int64_t i = threadIdx.x; i < words; i += CIW_TPB) s_bits[i] = bm[i];
        bm = s_bits;
    }
    __syncthreads();
    const CiTab T{offL, bounds, s_off, s_bnd, rows, nbs, lrows, lnbs};
    const int64_t N = s0 * s1 * s2;
    const int64_t nstat = (int64_t)gridDim.x * W;   // slots the waves own without asking
    const bool more = nstat < n;                      // block-uniform
    uint32_t *nx = next + b * CIB_NEXT_STRIDE;
    int64_t cur = (int64_t)blockIdx.x * W + w, end = cur + 1;   // the wave's run of slots
    while (cur < n) {   // wave-uniform; n <= V < 2^31 and at most one failed claim per wave: no wrap
        uint32_t mine = 0;
        if (more && lane == 0) mine = atomicAdd(nx, (uint32_t)CIB_CHUNK);   // the next run, in flight during this one
        for (; cur < end && cur < n; ++cur) {
            const int32_t v = list[b * V + cur];
            if (!CI_OK(v >= 0 && v < V, 13, v, V)) continue;
            const int64_t i = v / (s1 * s2), j = (v / s2) % s1, k = v % s2;
            const int64_t base = i + j * s0 + k * s0 * s1;   // px2vec (Fortran order, CI.py:65-68)
            const int32_t qstop = ci_walk_one(T, bm, words, base, N, lane);
            if (lane == 0) {
                shell16[b * V + v] = (int16_t)qstop;   // nbs <= 32767 (vh_ci_run)
                if (qstop >= 0 && CI_OK(qstop < nbs, 14, qstop, nbs)) {
                    if (lds_hist) atomicAdd(&s_hist[qstop], 1u);
                    else atomicAdd(&hist[b * nbs + qstop], 1u);
                } else {
                    atomicExch(&status[b], 1);
                }
            }
        }
        cur = more ? nstat + (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)mine) : n;
        end = cur + CIB_CHUNK;
    }
    if (lds_hist) {   // every wave of the workgroup comes here: nothing returns after the staging
        __syncthreads();
        for (int q = threadIdx.x; q < (int)nbs; q += CIW_TPB) {
            const uint32_t c = s_hist[q];
            if (c) atomicAdd(&hist[b * nbs + q], c);
        }
    }
}

// the workspace's zeroing in one launch (four hipMemsetAsync blits before: ~4 us each, r4ab)
__global__ void k_ci_clear(int32_t *status, unsigned long long *count, uint32_t *next, int64_t nb,
                           uint32_t *bits, int64_t nbits, uint32_t *hist, int64_t nhist) {
    const int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < nbits; i += st) bits[i] = 0u;
    for (int64_t i = i0; i < nhist; i += st) hist[i] = 0u;
    for (int64_t i = i0; i < nb; i += st) {
        status[i] = 0;
        count[i] = 0ull;
        if (next) next[i * CIB_NEXT_STRIDE] = 0u;
    }
}

// The 95th-percentile shell (Vent_Analysis.py:265-271): the first shell q whose cumulative count
// passes i95, one workgroup per volume -- each thread sums a run of consecutive shells, an
// exclusive scan of the run sums finds the run holding the crossing, and that run is walked (one
// thread per volume walked every shell serially: 16 us, r4ab).  Integer sums: order-free.
#define CIF_TPB 256
#define CIF_LDS 16384   // shells staged in LDS (64 KiB)
__global__ void __launch_bounds__(CIF_TPB) k_ci_finish(const uint32_t *hist, const unsigned long long *count,
                                                      const double *radii, int64_t nbs, double minvox,
                                                      int64_t nb, const int32_t *status, VolScalars *sc,
                                                      VolScalars *hsc) {
    __shared__ unsigned long long s_sum[CIF_TPB];
    __shared__ int s_hit;
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t D = (int64_t)count[b];
    if (t == 0) {
        const int32_t cs = status[b] ? VH_ERR_MAXRADIUS : (D == 0 ? VH_ERR_EMPTY : VH_OK);
        sc[b].n_ci = D;
        sc[b].ci_status = cs;
        sc[b].ci_scalar = 0.0;
        if (hsc) {   // the host's page-locked copy (vector stores over the link)
            hsc[b].n_ci = D;
            hsc[b].ci_status = cs;
            hsc[b].ci_scalar = 0.0;
        }
        s_hit = -1;
    }
    if (status[b] || D == 0) return;   // block-uniform
    const unsigned long long i95 = (unsigned long long)(int64_t)(0.95 * (double)D);
    const int64_t per = (nbs + CIF_TPB - 1) / CIF_TPB, q0 = t * per, q1 = min(q0 + per, nbs);
    // the histogram staged through LDS by coalesced loads first (one thread's run of dependent-
    // address loads took ~16 us, r4al), when it fits
    extern __shared__ uint32_t s_h[];
    const uint32_t *h = hist + b * nbs;
    if (nbs <= CIF_LDS) {
        for (int64_t q = t; q < nbs; q += CIF_TPB) s_h[q] = h[q];
        __syncthreads();
        h = s_h;
    }
    unsigned long long own = 0;
    for (int64_t q = q0; q < q1; ++q) own += h[q];
    s_sum[t] = own;
    __syncthreads();
    if (t == 0) {   // exclusive scan of the run sums (256 adds) and the run holding the crossing
        unsigned long long run = 0;
        for (int i = 0; i < CIF_TPB; ++i) {
            const unsigned long long v = s_sum[i];
            s_sum[i] = run;
            run += v;
            if (s_hit < 0 && run > i95) s_hit = i;
        }
    }
    __syncthreads();
    if (t == s_hit) {
        unsigned long long cum = s_sum[t];
        for (int64_t q = q0; q < q1; ++q) {
            cum += h[q];
            if (cum > i95) {
                if (!CI_OK(q < nbs, 10, q, nbs)) break;
                sc[b].ci_scalar = radii[q] * minvox;
                if (hsc) hsc[b].ci_scalar = radii[q] * minvox;
                break;
            }
        }
    }
}

__global__ void k_ci_scatter(const int32_t *shell_of, const uint8_t *defect, const double *radii,
                             int64_t nbs, double minvox, int64_t V, double *ci) {
    const int64_t b = blockIdx.y;
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= V) return;
    double r = 0.0;
    if (defect[b * V + v]) {
        const int32_t q = shell_of[b * V + v];
        r = q >= 0 && CI_OK(q < nbs, 11, q, nbs) ? radii[q] * minvox : 0.0;
    }
    ci[b * V + v] = r;
}

// vh_batch_download_ci's float64 map from the int16 shells (-1 off-defect and at the last radius:
// 0.0, as k_ci_scatter gives)
__global__ void k_ci_expand16(const int16_t *shell16, const double *radii, int64_t nbs, double minvox,
                              int64_t V, double *ci) {
    const int64_t b = blockIdx.y;
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int32_t q = shell16[b * V + v];
    ci[b * V + v] = q >= 0 && CI_OK(q < nbs, 15, q, nbs) ? radii[q] * minvox : 0.0;
}

// host: a compact sphere table uploaded once (vh_ci_table_create): the linear px2vec offsets of
// its rows for one (R, C) -- the stride of L = i + j R + k R C, CI.py:65-68 -- with duplicates
// marked, the shell boundaries and radii, all resident in HBM until vh_ci_table_destroy.
vh_ci_table *vh_ci_table_build(vh_ctx *ctx, int64_t R, int64_t C, const int16_t *offs, const uint8_t *dup,
                               int64_t rows, const int32_t *bounds, const double *radii, int64_t nbs) {
    if (!offs || !dup || !bounds || !radii || rows < 1 || nbs < 1 || R < 1 || C < 1)
        throw VhError{VH_ERR_ARG, "null buffer / empty table"};
    for (int64_t q = 0; q < nbs; ++q)
        if (bounds[q] < 1 || bounds[q] > rows || (q && bounds[q] <= bounds[q - 1]))
            throw VhError{VH_ERR_ARG, "sphere table bounds must be increasing in [1, rows]"};
    std::vector<int32_t> offL(rows);
    for (int64_t r = 0; r < rows; ++r)
        offL[r] = dup[r] ? CI_SENTINEL
                         : (int32_t)(offs[3 * r] + (int64_t)offs[3 * r + 1] * R + (int64_t)offs[3 * r + 2] * R * C);
    HIP_TRY(hipSetDevice(ctx->device));
    vh_ci_table *t = new vh_ci_table;
    t->ctx = ctx;
    t->R = R;
    t->C = C;
    t->rows = rows;
    t->nbs = nbs;
    try {
        t->d_offL.reserve((size_t)rows);
        t->d_bounds.reserve((size_t)nbs);
        t->d_radii.reserve((size_t)nbs);
        HIP_TRY(hipMemcpy(t->d_offL, offL.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->d_bounds, bounds, sizeof(int32_t) * nbs, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->d_radii, radii, sizeof(double) * nbs, hipMemcpyHostToDevice));
    } catch (...) {
        vh_ci_table_free(t);
        throw;
    }
    return t;
}

void vh_ci_table_free(vh_ci_table *t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    delete t;
}

// results stay on device (d_ci_shell, d_sc); the float64 CI map goes to d_ci (nb*V doubles) when
// given -- device memory, or a device-mapped page-locked host buffer the scatter writes across the
// link -- and the CI scalars also to h_sc (device-mapped host memory) when given.  Enqueued on the
// batch's stream; the caller synchronises.
//
// form 0 (vh_ci, vh_ci_tab): k_ci_walk, shells as int32 in d_ci_shell.  Forms 1 and 2 (vh_batch_ci):
// shells as int16 in d_ci_shell16, -1 off-defect, walked by k_ci_walk or by the batch form k_ci_walk_b.
void vh_ci_run(vh_batch *b, const vh_ci_table *t, double minvox, double *d_ci, VolScalars *h_sc, int form) {
    if (t->R != b->R || t->C != b->C) throw VhError{VH_ERR_ARG, "sphere table built for another (R, C)"};
    if (form && t->nbs > 32767) throw VhError{VH_ERR_ARG, "sphere table has more than 32767 shells: no int16 map"};
    hipStream_t st = b->stream;
    const int64_t words = (b->V + 31) / 32, rows = t->rows, nbs = t->nbs;
    // workspace owned by the batch (freed with it): no allocation, and nothing to leak, per call
    const size_t nb = (size_t)b->nb;
    b->d_ci_status.reserve(nb);
    b->d_ci_count.reserve(nb);
    int32_t *d_status = b->d_ci_status;
    unsigned long long *d_count = b->d_ci_count;
    b->d_bitmap.reserve(nb * words);
    b->d_ci_list.reserve(nb * b->V);
    if (!form) b->d_ci_shell.reserve(nb * b->V);
    if (form) {
        b->d_ci_shell16.reserve(nb * b->V);
        b->d_ci_next.reserve(CIB_NEXT_STRIDE * nb);
    }
    int16_t *d_s16 = form ? b->d_ci_shell16 : nullptr;
    b->d_ci_hist.reserve(nb * nbs);
    {
        const int64_t big = std::max<int64_t>(b->nb * words, b->nb * nbs);
        k_ci_clear<<<(unsigned)std::min<int64_t>((big + VH_TPB - 1) / VH_TPB, 1024), VH_TPB, 0, st>>>(
            d_status, d_count, form ? b->d_ci_next : nullptr, b->nb, b->d_bitmap, b->nb * words, b->d_ci_hist,
            b->nb * nbs);
        VH_CHECK_LAUNCH();
    }
    const dim3 vg((unsigned)((b->V + VH_TPB - 1) / VH_TPB), (unsigned)b->nb);
    k_ci_bitmap<<<vg, VH_TPB, 0, st>>>(b->d_defect, b->R, b->C, b->Z, b->V, words, b->d_bitmap,
                                       b->d_ci_list, d_count, d_s16);
    VH_CHECK_LAUNCH();
    if (form == 2) {
        ScopedKTimer tm(b, "ci_walk_b", 0.0);
        // CIB_WG_PER_CU workgroups per CU over the whole batch, at most CIB_G_MAX per study and never
        // more than V voxels could need (a workgroup past the study's defect count exits at once)
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->ctx->device));
        const int64_t gmax = std::min<int64_t>((b->V + CIW_TPB / 64 - 1) / (CIW_TPB / 64), 512);
        int64_t G = std::min<int64_t>((CIB_WG_PER_CU * (int64_t)cus + b->nb - 1) / b->nb, CIB_G_MAX);
        if (const char *e = getenv("VH_CI_B_G")) G = atoi(e);
        G = std::max<int64_t>(1, std::min<int64_t>(G, gmax));
        int hrows = CIB_ROWS;
        if (const char *e = getenv("VH_CI_B_ROWS")) hrows = std::max(256, std::min(CIW_ROWS, atoi(e) / 256 * 256));
        const int lds_hist = nbs <= CIB_HIST_MAX ? 1 : 0;
        const size_t fixed = sizeof(uint32_t) * (size_t)(hrows + CIB_NBS + (lds_hist ? nbs : 0));
        const int stage_bits = fixed + sizeof(uint32_t) * (size_t)words <= CIW_LDS_MAX ? 1 : 0;
        vh_set_max_lds((const void *)k_ci_walk_b, CIW_LDS_MAX);
        k_ci_walk_b<<<dim3((unsigned)G, (unsigned)b->nb), CIW_TPB,
                      fixed + (stage_bits ? sizeof(uint32_t) * (size_t)words : 0), st>>>(
            b->d_bitmap, b->d_ci_list, d_count, b->d_ci_next, t->d_offL, rows, t->d_bounds, nbs, b->R, b->C,
            b->Z, b->V, words, hrows, lds_hist, stage_bits, d_s16, b->d_ci_hist, d_status);
        VH_CHECK_LAUNCH();
    } else {
        ScopedKTimer tm(b, "ci_walk", 0.0);
        // one wave per defect voxel, 16 per block; blocks stride over the defect list past 512 per
        // volume (two per CU), and a block past the volume's defect count exits before staging
        const int64_t wg = std::min<int64_t>((b->V + CIW_TPB / 64 - 1) / (CIW_TPB / 64), 512);
        const size_t fixed = sizeof(int32_t) * (CIW_ROWS + CIW_NBS);
        const int stage_bits = fixed + sizeof(uint32_t) * (size_t)words <= CIW_LDS_MAX ? 1 : 0;
        vh_set_max_lds((const void *)k_ci_walk, CIW_LDS_MAX);
        k_ci_walk<<<dim3((unsigned)wg, (unsigned)b->nb), CIW_TPB,
                    fixed + (stage_bits ? sizeof(uint32_t) * (size_t)words : 0), st>>>(
            b->d_bitmap, b->d_ci_list, d_count, t->d_offL, rows, t->d_bounds, nbs, b->R, b->C, b->Z, b->V,
            words, stage_bits, b->d_ci_shell, d_s16, b->d_ci_hist, d_status);
        VH_CHECK_LAUNCH();
    }
    vh_set_max_lds((const void *)k_ci_finish, (int)(sizeof(uint32_t) * CIF_LDS + 4096));
    k_ci_finish<<<(unsigned)b->nb, CIF_TPB, nbs <= CIF_LDS ? sizeof(uint32_t) * (size_t)nbs : 0, st>>>(
        b->d_ci_hist, d_count, t->d_radii, nbs, minvox, b->nb, d_status, b->d_sc, h_sc);
    VH_CHECK_LAUNCH();
    if (d_ci && !form) {
        k_ci_scatter<<<vg, VH_TPB, 0, st>>>(b->d_ci_shell, b->d_defect, t->d_radii, nbs, minvox, b->V, d_ci);
        VH_CHECK_LAUNCH();
    }
}

// VH_CI_FORM, read at call time like VH_N4_MODE: 1 = k_ci_walk on the resident batch, 2 = the batch
// form k_ci_walk_b, unset / 0 = auto (DESIGN 4.4 has the measurement behind the rule)
int vh_ci_batch_form(const vh_batch *b) {
    const char *e = getenv("VH_CI_FORM");
    const int f = e ? atoi(e) : 0;
    if (f == 1 || f == 2) return f;
    return b->nb >= CIB_AUTO_MIN_NB ? 2 : 1;
}

void vh_ci_expand(vh_batch *b, double *d_ci) {
    const dim3 vg((unsigned)((b->V + VH_TPB - 1) / VH_TPB), (unsigned)b->nb);
    k_ci_expand16<<<vg, VH_TPB, 0, b->stream>>>(b->d_ci_shell16, b->d_ci_radii, b->state.ci_nbs(), b->state.ci_minvox(), b->V,
                                                d_ci);
    VH_CHECK_LAUNCH();
}

// VH_DEBUG_BOUNDS: the first recorded violation of the CI kernels since the last check, raised
// (after the caller's stream sync); a no-op in release builds
void vh_ci_debug_check() {
#ifdef VH_DEBUG_BOUNDS
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ci_dbg), sizeof h, 0, hipMemcpyDeviceToHost));
    if (h[0]) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_ci_dbg), z, sizeof z, 0, hipMemcpyHostToDevice));
        throw VhError{VH_ERR_HIP, "CI bounds check: site " + std::to_string(h[0]) + " index " +
                                      std::to_string((long long)h[1]) + " extent " + std::to_string((long long)h[2])};
    }
#endif
}
