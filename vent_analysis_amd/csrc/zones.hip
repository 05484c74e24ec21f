// zones.hip -- the regional analysis of a resident batch (vh_batch_zones): a zone map of every study,
// geometric (thirds, left / right, a grid of parts over the mask's bounding box) or the caller's
// labels, and per zone the counts of mask, defect and linear-binning class voxels, the histogram of
// the normalised signal and its fixed-point sum.  Four kernels on the batch's stream, no host wait:
//   k_zn_profile  mask -> Pr, Pc, Pz per study (the on voxels of every row, column and slice)
//   k_zn_tables   the profiles -> the bounds, the split column and the part of every index (zones_host.h)
//   k_zn_map      the tables (or the uploaded labels) and the mask -> the zone byte of every voxel
//   k_zn_count    N4 (4 B), mask, defect, LB class, zone (1 B each) -> the counts
// Every accumulation is an integer add, so no result depends on the order of the adds.
// The three sweeps share one decomposition: a workgroup owns ZN_TPB consecutive (column, slice) pairs j
// and a slab of SL rows; thread t walks the rows of its pair j, so consecutive threads read consecutive
// bytes, a thread's column and slice never change, and its zone changes only where the row part does.
#include <algorithm>

#include "vh_internal.h"
#include "zones_host.h"

#define ZN_TPB 256
#define ZN_UNROLL 8          // rows per thread with their loads in flight together
#ifndef ZN_PROF_LOADS
#define ZN_PROF_LOADS 8      // rows of the profile sweep with their loads in flight together (divides 32;
#endif                       // 8: 265 us for the whole call on the 256 x 128x128x24 batch, 32: 285 us, alternating)
#define ZN_MAX_SL 256        // the most rows of a slab (a multiple of 32)
#define ZN_TAB_LDS 12288     // k_zn_tables stages a study's profiles in LDS up to this many entries
#define ZN_NC 10             // a zone's LDS count columns: the 8 of VH_ZONE_COLS, n_below, n_over

struct ZnGeom {
    int R, C, Z;
    int64_t CZ, V;
    int ncb;                 // blocks of ZN_TPB (column, slice) pairs
    int SL, slabs;           // rows per slab (a multiple of 32, <= ZN_MAX_SL), slabs per study
};

// about 4096 workgroups in all where the rows allow it: every workgroup of k_zn_count flushes up to
// (K + 1) (n_bins + 12) counts, so few rows per workgroup would make the flush the larger part
static ZnGeom zn_geometry(const vh_batch *b) {
    ZnGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    g.CZ = b->CZ; g.V = b->V;
    g.ncb = (int)((b->CZ + ZN_TPB - 1) / ZN_TPB);
    const int64_t want = std::max<int64_t>(1, (4096 + (int64_t)g.ncb * b->nb - 1) / ((int64_t)g.ncb * b->nb));
    const int64_t rows = (b->R + want - 1) / want;
    g.SL = (int)std::min<int64_t>(ZN_MAX_SL, std::max<int64_t>(32, (rows + 31) / 32 * 32));
    g.slabs = (g.R + g.SL - 1) / g.SL;
    return g;
}
static int64_t zn_blocks(const ZnGeom &g) { return (int64_t)g.ncb * g.slabs; }

// grid (ncb * slabs, nb).  A row's count: the wave's ballot, kept by lane (row % 32) until 32 rows are
// done; a thread's own count over the slab is its (column, slice) pair's, added to the column and the
// slice once.  LDS -> global integer atomics on the nonzero entries, once per workgroup; with Z >=
// ZN_TPB every thread of a workgroup has a slice of its own and adds to the global counter itself.
__global__ void __launch_bounds__(ZN_TPB) k_zn_profile(const uint8_t *__restrict__ mask, ZnGeom g, uint32_t *prof) {
    __shared__ uint32_t s_row[ZN_MAX_SL], s_col[ZN_TPB + 1], s_sl[ZN_TPB];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t b = blockIdx.y;
    const int cb = blockIdx.x % g.ncb, slab = blockIdx.x / g.ncb;
    const int r0 = slab * g.SL, r1 = min(g.R, r0 + g.SL);
    s_row[t] = 0u; s_col[t] = 0u; s_sl[t] = 0u;
    if (t == 0) s_col[ZN_TPB] = 0u;
    __syncthreads();
    const int64_t j = (int64_t)cb * ZN_TPB + t;
    const bool valid = j < g.CZ;
    const uint32_t c = valid ? (uint32_t)j / (uint32_t)g.Z : 0u, z = valid ? (uint32_t)j - c * (uint32_t)g.Z : 0u;
    const uint32_t c0 = (uint32_t)((int64_t)cb * ZN_TPB) / (uint32_t)g.Z;
    const uint8_t *m = mask + b * g.V + (valid ? j : 0);
    const int L = g.R + g.C + g.Z;
    uint32_t *P = prof + b * L;
    uint32_t cnt = 0u;
    for (int rr = 0; rr < g.SL && r0 + rr < r1; rr += 32) {
        uint32_t rowcnt = 0u;
#pragma unroll
        for (int q0 = 0; q0 < 32; q0 += ZN_PROF_LOADS) {
            uint32_t mv[ZN_PROF_LOADS];
#pragma unroll
            for (int q = 0; q < ZN_PROF_LOADS; ++q)   // (no load is conditional, so all are in flight together: a
                mv[q] = m[(int64_t)min(r0 + rr + q0 + q, r1 - 1) * g.CZ];   // row past the slab reads its last row)
#pragma unroll
            for (int q = 0; q < ZN_PROF_LOADS; ++q) {
                const bool on = valid && r0 + rr + q0 + q < r1 && mv[q] != 0u;
                const uint32_t n = (uint32_t)__popcll(__ballot(on));
                rowcnt += lane == q0 + q ? n : 0u;
                cnt += on;
            }
        }
        if (lane < 32 && rowcnt) atomicAdd(&s_row[rr + lane], rowcnt);   // (rr + lane < SL: a multiple of 32)
    }
    if (cnt) {
        atomicAdd(&s_col[c - c0], cnt);   // (c - c0 <= (ZN_TPB - 1) / Z + 1 <= ZN_TPB)
        if (g.Z < ZN_TPB) atomicAdd(&s_sl[z], cnt);
        else atomicAdd(&P[g.R + g.C + z], cnt);
    }
    __syncthreads();
    if (r0 + t < r1 && s_row[t]) atomicAdd(&P[r0 + t], s_row[t]);
    for (int i = t; i < ZN_TPB + 1; i += ZN_TPB)
        if (c0 + i < (uint32_t)g.C && s_col[i]) atomicAdd(&P[g.R + c0 + i], s_col[i]);
    if (g.Z < ZN_TPB && t < g.Z && s_sl[t]) atomicAdd(&P[g.R + g.C + t], s_sl[t]);
}

// One workgroup per study.  The bounds of the three axes by one thread each (waves 0..2), the split by
// wave 3's first thread; then the part tables: by extent every thread takes indices, by count the
// running sum is one thread's per axis.  staged: the study's profiles are copied to LDS first.
__global__ void __launch_bounds__(ZN_TPB) k_zn_tables(const uint32_t *__restrict__ prof, int R, int C, int Z, int pr,
                                                      int pc, int pz, int lateral, int by, int geometric, int staged,
                                                      uint8_t *tab, int32_t *geom) {
    extern __shared__ __align__(16) uint32_t s_prof[];
    __shared__ int32_t s_lo[3], s_hi[3], s_s;
    __shared__ long long s_tot[3];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int L = R + C + Z;
    const uint32_t *P = prof + b * L;
    if (staged) {
        for (int i = t; i < L; i += ZN_TPB) s_prof[i] = P[i];
        __syncthreads();
        P = s_prof;
    }
    uint8_t *T = tab + b * L;
    const int n[3] = {R, C, Z}, off[3] = {0, R, R + C}, p[3] = {pr, pc, pz};
    if ((t & 63) == 0 && t < 192) {
        const int a = t >> 6;
        int32_t lo, hi;
        int64_t tot;
        zn_bounds(P + off[a], n[a], lo, hi, tot);
        s_lo[a] = lo; s_hi[a] = hi; s_tot[a] = tot;
    }
    __syncthreads();
    if (t == 192) s_s = (geometric && lateral) ? zn_split(P + R, s_lo[1], s_hi[1]) : -1;
    __syncthreads();
    if (t == 0) {
        int32_t *gm = geom + b * 8;
        for (int a = 0; a < 3; ++a) { gm[2 * a] = s_lo[a]; gm[2 * a + 1] = s_hi[a]; }
        gm[6] = s_s;
        gm[7] = 0;
    }
    if (!geometric) return;
    for (int a = 0; a < 3; ++a) {
        uint8_t *Ta = T + off[a];
        if (a == 1 && lateral) {
            const int s = s_s;
            for (int i = t; i < C; i += ZN_TPB) Ta[i] = i >= s;
        } else if (by == ZN_EXTENT) {
            const int32_t lo = s_lo[a], w = s_hi[a] - lo + 1;
            for (int i = t; i < n[a]; i += ZN_TPB) Ta[i] = (uint8_t)zn_part_extent(i, lo, w, p[a]);
        } else if (t == 64 * a) {
            zn_axis_parts(P + off[a], n[a], p[a], ZN_COUNT, s_lo[a], s_hi[a], s_tot[a], Ta);
        }
    }
}

// grid (ncb * slabs, nb).  Geometric: zone = 1 + (part_r nc + col) pz + part_z on the mask, 0 off it.
// LABELS: map holds the caller's bytes; a byte 1..K on the mask stays, every other becomes 0.
template <bool LABELS>
__global__ void __launch_bounds__(ZN_TPB) k_zn_map(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ tab,
                                                   ZnGeom g, int nc, int pz, int K, uint8_t *map) {
    const int t = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int cb = blockIdx.x % g.ncb, slab = blockIdx.x / g.ncb;
    const int r0 = slab * g.SL, r1 = min(g.R, r0 + g.SL);
    const int64_t j = (int64_t)cb * ZN_TPB + t;
    if (j >= g.CZ) return;
    const uint8_t *m = mask + b * g.V + j;
    uint8_t *o = map + b * g.V + j;
    const uint8_t *T = tab + b * (g.R + g.C + g.Z);
    uint32_t colz = 0u;
    if (!LABELS) {
        const uint32_t c = (uint32_t)j / (uint32_t)g.Z, z = (uint32_t)j - c * (uint32_t)g.Z;
        colz = (uint32_t)T[g.R + c] * (uint32_t)pz + (uint32_t)T[g.R + g.C + z];
    }
    const uint32_t rowf = (uint32_t)(nc * pz);
    int r = r0;
    for (; r + ZN_UNROLL <= r1; r += ZN_UNROLL) {
        uint32_t mv[ZN_UNROLL], lv[ZN_UNROLL];
#pragma unroll
        for (int q = 0; q < ZN_UNROLL; ++q) {
            const int64_t i = (int64_t)(r + q) * g.CZ;
            mv[q] = m[i];
            lv[q] = LABELS ? (uint32_t)o[i] : (uint32_t)T[r + q];
        }
#pragma unroll
        for (int q = 0; q < ZN_UNROLL; ++q) {
            const uint32_t zone = LABELS ? ((lv[q] >= 1u && lv[q] <= (uint32_t)K) ? lv[q] : 0u)
                                         : 1u + lv[q] * rowf + colz;
            o[(int64_t)(r + q) * g.CZ] = (uint8_t)(mv[q] ? zone : 0u);
        }
    }
    for (; r < r1; ++r) {
        const int64_t i = (int64_t)r * g.CZ;
        const uint32_t l = LABELS ? (uint32_t)o[i] : (uint32_t)T[r];
        const uint32_t zone = LABELS ? ((l >= 1u && l <= (uint32_t)K) ? l : 0u) : 1u + l * rowf + colz;
        o[i] = (uint8_t)(m[i] ? zone : 0u);
    }
}

// a thread's counters of its current zone -> the workgroup's LDS rows, the nonzero ones
__device__ __forceinline__ void zn_flush(uint32_t zone, uint32_t (&c)[ZN_NC], unsigned long long &fx, uint32_t *s_cnt,
                                         unsigned long long *s_fx) {
#pragma unroll
    for (int k = 0; k < ZN_NC; ++k)
        if (c[k]) {
            atomicAdd(&s_cnt[zone * ZN_NC + k], c[k]);
            c[k] = 0u;
        }
    if (fx) {
        atomicAdd(&s_fx[zone], fx);
        fx = 0ull;
    }
}

// One on voxel.  nv = x / d is IEEE float32 division and nv * scale one float32 multiply
// (-ffp-contract=off), the expressions of k_dist; the fixed point is k_het's.
__device__ __forceinline__ void zn_voxel(float x, uint32_t df, uint32_t l, uint32_t zone, float d, float hi, float scale,
                                         int n_bins, uint32_t &cur, uint32_t (&c)[ZN_NC], unsigned long long &fx,
                                         uint32_t *s_cnt, unsigned long long *s_fx, uint32_t *s_hist) {
    if (zone != cur) {
        zn_flush(cur, c, fx, s_cnt, s_fx);
        cur = zone;
    }
    c[0] += 1u;
    c[1] += df != 0u;
#pragma unroll
    for (uint32_t k = 1; k <= 6; ++k) c[k + 1] += l == k;   // (a class byte above 6 counts nowhere)
    const float nv = x / d;
    if (nv >= 0.0f && nv < hi) {
        int bi = (int)(nv * scale);
        bi = bi < 0 ? 0 : bi > n_bins - 1 ? n_bins - 1 : bi;
        atomicAdd(&s_hist[zone * n_bins + bi], 1u);
        fx += (unsigned long long)(long long)(nv * 16777216.0f);
    } else if (nv < 0.0f) {
        c[8] += 1u;
    } else {   // nv >= hi, NaN: whatever a zero, infinite or NaN divisor gives included
        c[9] += 1u;
    }
}

// grid (ncb * slabs, nb), LDS (K + 1) (n_bins + 12) words: s_fx [K1] (64-bit), s_cnt [K1][ZN_NC], s_hist
// [K1][n_bins].  A thread keeps the ten counters and the fixed-point sum of its current zone in
// registers and adds them to LDS where its zone changes and at its end; the histogram bin is an LDS
// atomic per voxel.  n_in of a zone is its mask count less n_below and n_over.  The workgroup's counts
// go out once: LDS -> global integer atomics on the nonzero entries.
__global__ void __launch_bounds__(ZN_TPB) k_zn_count(const float *__restrict__ n4, const uint8_t *__restrict__ mask,
                                                     const uint8_t *__restrict__ defect,
                                                     const uint8_t *__restrict__ lb, const uint8_t *__restrict__ zmap,
                                                     const VolScalars *sc, ZnGeom g, int norm, int n_bins, float hi,
                                                     float scale, int K1, unsigned long long *counts, uint32_t *hist,
                                                     unsigned long long *stats) {
    extern __shared__ __align__(16) uint32_t s_zn[];
    unsigned long long *s_fx = reinterpret_cast<unsigned long long *>(s_zn);   // [K1]
    uint32_t *s_cnt = s_zn + 2 * K1;                                            // [K1][ZN_NC]
    uint32_t *s_hist = s_cnt + ZN_NC * K1;                                      // [K1][n_bins]
    const int t = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int cb = blockIdx.x % g.ncb, slab = blockIdx.x / g.ncb;
    const int r0 = slab * g.SL, r1 = min(g.R, r0 + g.SL);
    const int nw = K1 * (n_bins + 12);
    for (int i = t; i < nw; i += ZN_TPB) s_zn[i] = 0u;
    __syncthreads();
    const float d = norm == VH_NORM_MEAN ? sc[b].mean_anchor : sc[b].p99;
    const int64_t j = (int64_t)cb * ZN_TPB + t;
    if (j < g.CZ) {
        const int64_t base = b * g.V + j;
        const float *x = n4 + base;
        const uint8_t *mk = mask + base, *df = defect + base, *cl = lb + base, *zn = zmap + base;
        uint32_t cur = 0u, c[ZN_NC] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        unsigned long long fx = 0ull;
        int r = r0;
        for (; r + ZN_UNROLL <= r1; r += ZN_UNROLL) {
            float xv[ZN_UNROLL];
            uint32_t mv[ZN_UNROLL], dv[ZN_UNROLL], lv[ZN_UNROLL], zv[ZN_UNROLL];
#pragma unroll
            for (int q = 0; q < ZN_UNROLL; ++q) {
                const int64_t i = (int64_t)(r + q) * g.CZ;
                xv[q] = x[i]; mv[q] = mk[i]; dv[q] = df[i]; lv[q] = cl[i]; zv[q] = zn[i];
            }
#pragma unroll
            for (int q = 0; q < ZN_UNROLL; ++q)
                if (mv[q])   // (a zone byte is at most K by construction; the bound keeps LDS safe regardless)
                    zn_voxel(xv[q], dv[q], lv[q], zv[q] < (uint32_t)K1 ? zv[q] : 0u, d, hi, scale, n_bins, cur, c, fx,
                             s_cnt, s_fx, s_hist);
        }
        for (; r < r1; ++r) {
            const int64_t i = (int64_t)r * g.CZ;
            if (mk[i]) {
                const uint32_t z = zn[i];
                zn_voxel(x[i], df[i], cl[i], z < (uint32_t)K1 ? z : 0u, d, hi, scale, n_bins, cur, c, fx, s_cnt, s_fx,
                         s_hist);
            }
        }
        zn_flush(cur, c, fx, s_cnt, s_fx);
    }
    __syncthreads();
    for (int i = t; i < K1 * ZN_NC; i += ZN_TPB) {
        const uint32_t v = s_cnt[i];
        if (!v) continue;
        const int k = i / ZN_NC, col = i - k * ZN_NC;
        if (col < VH_ZONE_COLS) atomicAdd(&counts[(b * K1 + k) * VH_ZONE_COLS + col], (unsigned long long)v);
        else atomicAdd(&stats[(b * K1 + k) * 4 + (col - VH_ZONE_COLS + 1)], (unsigned long long)v);
    }
    for (int k = t; k < K1; k += ZN_TPB) {
        const uint32_t n_in = s_cnt[k * ZN_NC] - s_cnt[k * ZN_NC + 8] - s_cnt[k * ZN_NC + 9];
        if (n_in) atomicAdd(&stats[(b * K1 + k) * 4], (unsigned long long)n_in);
        if (s_fx[k]) atomicAdd(&stats[(b * K1 + k) * 4 + 3], s_fx[k]);
    }
    for (int i = t; i < K1 * n_bins; i += ZN_TPB)
        if (s_hist[i]) atomicAdd(&hist[b * K1 * n_bins + i], s_hist[i]);
}

bool vh_zones_takes(const vh_batch *b) {   // the grid: x in threads below 2^32, y
    return zn_blocks(zn_geometry(b)) < ((int64_t)1 << 24) && b->nb <= 65535;
}

void vh_zones_launch(vh_batch *b, bool labels, int K, const int32_t parts[3], int lateral, int by, int norm,
                     int n_bins, float hi, float scale) {
    hipStream_t st = b->stream;
    const ZnGeom g = zn_geometry(b);
    const size_t nb = (size_t)b->nb, L = (size_t)(b->R + b->C + b->Z);
    const int K1 = K + 1;
    HIP_TRY(hipMemsetAsync(b->d_zn_prof, 0, sizeof(uint32_t) * nb * L, st));
    HIP_TRY(hipMemsetAsync(b->d_zn_counts, 0, sizeof(unsigned long long) * nb * K1 * VH_ZONE_COLS, st));
    HIP_TRY(hipMemsetAsync(b->d_zn_hist, 0, sizeof(uint32_t) * nb * K1 * n_bins, st));
    HIP_TRY(hipMemsetAsync(b->d_zn_stats, 0, sizeof(unsigned long long) * nb * K1 * 4, st));
    // the mask once for the profiles; mask (and labels) in, zone out for the map; N4, mask, defect, LB
    // class and zone for the counts
    ScopedKTimer tm(b, "zones_b", (labels ? 12.0 : 11.0) * (double)b->nb * (double)b->V);
    const dim3 grid((unsigned)zn_blocks(g), (unsigned)b->nb, 1);
    k_zn_profile<<<grid, ZN_TPB, 0, st>>>(b->d_mask, g, b->d_zn_prof);
    VH_CHECK_LAUNCH();
    const int staged = L <= ZN_TAB_LDS;
    const int nc = lateral ? 2 : parts[1];
    k_zn_tables<<<(unsigned)b->nb, ZN_TPB, staged ? sizeof(uint32_t) * L : 0, st>>>(
        b->d_zn_prof, g.R, g.C, g.Z, parts[0], parts[1], parts[2], lateral, by, labels ? 0 : 1, staged, b->d_zn_tab,
        b->d_zn_geom);
    VH_CHECK_LAUNCH();
    if (labels)
        k_zn_map<true><<<grid, ZN_TPB, 0, st>>>(b->d_mask, b->d_zn_tab, g, nc, parts[2], K, b->d_zn_map);
    else
        k_zn_map<false><<<grid, ZN_TPB, 0, st>>>(b->d_mask, b->d_zn_tab, g, nc, parts[2], K, b->d_zn_map);
    VH_CHECK_LAUNCH();
    const size_t lds = sizeof(uint32_t) * (size_t)K1 * ((size_t)n_bins + 12);
    k_zn_count<<<grid, ZN_TPB, lds, st>>>(b->n4_last(), b->d_mask, b->d_defect, b->d_lb, b->d_zn_map, b->d_sc, g, norm,
                                          n_bins, hi, scale, K1, b->d_zn_counts, b->d_zn_hist, b->d_zn_stats);
    VH_CHECK_LAUNCH();
}
