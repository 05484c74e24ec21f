// resample.hip -- the proton resampled from its own grid onto the batch's (vh_batch_resample_proton);
// the spec is in include/vent_hip.h.  One fused kernel: a workgroup owns one study, a band of
// destination rows and a tile of destination columns and slices.  It runs the z- and c-passes of the
// source rows the band needs into LDS, then the r-pass from LDS.  The nested sum of the spec is exactly
// separable, so the staging changes no bit; every multiply and add is rounded on its own.
#include <algorithm>
#include <climits>

#include "vh_internal.h"

#define RS_TPB 256
#define RS_TAPS VH_RESAMPLE_TAPS
#define RS_WP (RS_TAPS + 1)        // words between the weights of neighbouring indices in LDS: lanes with
                                   // consecutive slices read slot k of theirs from different banks
#define RS_TILE 1024               // destination (column, slice) pairs of a tile at most
#define RS_TZ 64                   // slices of a tile at most
#define RS_TC 256                  // columns of a tile at most: the tables take 11 words per column and slice
#define RS_BAND 16                 // destination rows of a band at most
#define RS_LDS_MAX (64 * 1024)     // what a launch takes without MaxDynamicSharedMemorySize
#define RS_LDS_DEFAULT (40 * 1024) // the budget the band is sized to (VH_RS_LDS_KB overrides it)
#define RS_INFLIGHT 16             // reads a thread of the one-z-tap forms has in flight (taps x source rows);
                                   // with 32 the bench shape took 0.74 ms against 0.73
#define RS_LDS_STATIC (4 * RS_BAND * (RS_TAPS + 2))   // the band's r-table, beside the dynamic part

// LDS of a workgroup: the staged rows [span][TC TZ], then per tile column and per tile slice the 8
// weights (pitch RS_WP), first and count
static size_t rs_lds_dynamic(int span, int TC, int TZ) {
    return sizeof(float) * ((size_t)span * TC * TZ + (size_t)(RS_WP + 2) * (TC + TZ));
}
static size_t rs_lds_bytes(int span, int TC, int TZ) { return rs_lds_dynamic(span, TC, TZ) + RS_LDS_STATIC; }

// grid (bands x column tiles x slice tiles, nb).  KC > 0: no slice of the batch has more than KZ z-taps and
// no column more than KC c-taps; the taps of a pair in a source row are then read as KC x KZ loads that do
// not wait for one another (a tap past the pair's count re-reads its last one and is not added), over
// several source rows at a time.  KC 0: any tables, a tap at a time.
template <int KC, int KZ>
__global__ void __launch_bounds__(RS_TPB) k_resample_b(const float *__restrict__ src, float *__restrict__ dst,
                                                       const int32_t *__restrict__ tab, int R, int C, int Z,
                                                       RsPlan p, unsigned long long *ks) {
    extern __shared__ float s_rs[];
    kst_begin(ks);
    const int tid = threadIdx.x;
    const int pe = p.TC * p.TZ;
    float *s_wc = s_rs + (size_t)p.span * pe;
    float *s_wz = s_wc + RS_WP * p.TC;
    int32_t *s_fc = reinterpret_cast<int32_t *>(s_wz + RS_WP * p.TZ);
    int32_t *s_kc = s_fc + p.TC;
    int32_t *s_fz = s_kc + p.TC;
    int32_t *s_kz = s_fz + p.TZ;

    int t = (int)blockIdx.x;
    const int tz = t % p.ntz; t /= p.ntz;
    const int tc = t % p.ntc;
    const int band = t / p.ntc;
    const int r0 = band * p.BR, nr = min(p.BR, R - r0);
    const int c0 = tc * p.TC, nc = min(p.TC, C - c0);
    const int z0 = tz * p.TZ, nz = min(p.TZ, Z - z0);
    const int ne = nc * nz;

    // the study's tables: per axis first [n], count [n], weight [n][8]
    const int32_t *tr = tab + (int64_t)blockIdx.y * 10 * ((int64_t)R + C + Z);
    const int32_t *tcx = tr + 10 * (int64_t)R, *tzx = tcx + 10 * (int64_t)C;
    const float *wr = reinterpret_cast<const float *>(tr + 2 * (int64_t)R);
    const float *wc = reinterpret_cast<const float *>(tcx + 2 * (int64_t)C);
    const float *wz = reinterpret_cast<const float *>(tzx + 2 * (int64_t)Z);

    __shared__ int32_t s_fr[RS_BAND], s_kr[RS_BAND];   // the band's r-table
    __shared__ float s_wr[RS_BAND * RS_TAPS];
    if (tid < nr) { s_fr[tid] = tr[r0 + tid]; s_kr[tid] = tr[R + r0 + tid]; }
    if (tid < nr * RS_TAPS) s_wr[tid] = wr[(int64_t)r0 * RS_TAPS + tid];
    for (int i = tid; i < nc; i += RS_TPB) { s_fc[i] = tcx[c0 + i]; s_kc[i] = tcx[C + c0 + i]; }
    for (int i = tid; i < nz; i += RS_TPB) { s_fz[i] = tzx[z0 + i]; s_kz[i] = tzx[Z + z0 + i]; }
    for (int i = tid; i < nc * RS_TAPS; i += RS_TPB)
        s_wc[(i / RS_TAPS) * RS_WP + i % RS_TAPS] = wc[(int64_t)c0 * RS_TAPS + i];
    for (int i = tid; i < nz * RS_TAPS; i += RS_TPB)
        s_wz[(i / RS_TAPS) * RS_WP + i % RS_TAPS] = wz[(int64_t)z0 * RS_TAPS + i];

    // the source rows of the band: base .. end - 1 (uniform; the host sized span from the same tables, so
    // end - base <= p.span)
    int base = INT_MAX, end = 0;
    for (int i = 0; i < nr; ++i) {
        const int k = tr[R + r0 + i];
        if (k > 0) {
            const int f = tr[r0 + i];
            base = min(base, f);
            end = max(end, f + k);
        }
    }
    const int rows = end > base ? min(end - base, p.span) : 0;
    if (rows == 0) base = 0;
    __syncthreads();

    // z- and c-pass: row jl of the stage holds, for every (c, z) of the tile, the c-sum of source row
    // base + jl.  The taps of a table lie inside the source, so every read does
    const float *S = src + (int64_t)blockIdx.y * p.Rs * p.Cs * p.Zs;
    for (int e = tid; e < ne; e += RS_TPB) {
        const int cl = e / nz, zl = e - cl * nz;
        const int fc = s_fc[cl], kc = s_kc[cl], fz = s_fz[zl], kz = s_kz[zl];
        const float *wcl = s_wc + cl * RS_WP, *wzl = s_wz + zl * RS_WP;
        const float *at = S + ((int64_t)base * p.Cs + fc) * p.Zs + fz;
        if constexpr (KC > 0) {
            // (with no tap at all, first is 0: the address is inside the source and what it holds is not added)
            int off[KC];
            float w[KC];
#pragma unroll
            for (int a = 0; a < KC; ++a) {
                const int aa = max(min(a, kc - 1), 0);
                off[a] = aa * p.Zs;
                w[a] = wcl[aa];
            }
            int zo[KZ];
            float wk[KZ];
#pragma unroll
            for (int k = 0; k < KZ; ++k) {
                zo[k] = max(min(k, kz - 1), 0);
                wk[k] = wzl[zo[k]];
            }
            // source rows whose reads are in flight together
            constexpr int ROWS = RS_INFLIGHT / (KC * KZ) > 0 ? RS_INFLIGHT / (KC * KZ) : 1;
#pragma unroll ROWS
            for (int jl = 0; jl < rows; ++jl) {
                const float *row = at + (int64_t)jl * p.Cs * p.Zs;
                float v[KC][KZ];
#pragma unroll
                for (int a = 0; a < KC; ++a)
#pragma unroll
                    for (int k = 0; k < KZ; ++k) v[a][k] = row[off[a] + zo[k]];
                float ac = 0.0f;
#pragma unroll
                for (int a = 0; a < KC; ++a) {
                    float az = 0.0f;
#pragma unroll
                    for (int k = 0; k < KZ; ++k)
                        if (k < kz) az = __fadd_rn(az, __fmul_rn(wk[k], v[a][k]));
                    if (a < kc) ac = __fadd_rn(ac, __fmul_rn(w[a], az));
                }
                s_rs[jl * pe + e] = ac;
            }
        } else {
            for (int jl = 0; jl < rows; ++jl, at += (int64_t)p.Cs * p.Zs) {
                float ac = 0.0f;
                for (int a = 0; a < kc; ++a) {
                    const float *col = at + (int64_t)a * p.Zs;
                    float az = 0.0f;
                    for (int k = 0; k < kz; ++k) az = __fadd_rn(az, __fmul_rn(wzl[k], col[k]));
                    ac = __fadd_rn(ac, __fmul_rn(wcl[a], az));
                }
                s_rs[jl * pe + e] = ac;
            }
        }
    }
    __syncthreads();

    // r-pass, from the stage: a row with no tap gives +0.0f
    float *D = dst + (int64_t)blockIdx.y * R * C * Z;
    for (int i = tid; i < nr * ne; i += RS_TPB) {
        const int rl = i / ne, e = i - rl * ne;
        const int r = r0 + rl;
        const int f = s_fr[rl];
        int k = s_kr[rl];
        if (f < base || f - base + k > rows) k = 0;   // (never: the band's rows cover every tap of its rows)
        const float *w = s_wr + rl * RS_TAPS;
        const float *st = s_rs + (k > 0 ? (f - base) * pe : 0) + e;
        float ar = 0.0f;
        for (int a = 0; a < k; ++a) ar = __fadd_rn(ar, __fmul_rn(w[a], st[a * pe]));
        const int cl = e / nz, zl = e - cl * nz;
        D[((int64_t)r * C + c0 + cl) * Z + z0 + zl] = ar;
    }
    kst_end(ks);
}

// The tile: slices in equal chunks of at most RS_TZ, columns in equal chunks of at most RS_TC so that a
// tile has at most RS_TILE pairs.  The band: the most rows, up to RS_BAND, whose largest stage over every
// study and band fits the LDS budget.  One row always fits: its stage is at most 8 source rows (the taps
// of one index), 32 KiB at RS_TILE pairs, and the tables of the largest tile take 11 words per column and
// per slice, 13.75 KiB.  (VH_RS_LDS_KB, 1..64, is a diagnostics variable like VH_SYNC_CHECK: it sets the
// budget for scripts/resample_bench.py's sweep and for the test of the band logic; no result depends on it.)
static_assert(sizeof(float) * (RS_TAPS * RS_TILE + (RS_WP + 2) * (RS_TC + RS_TZ)) + RS_LDS_STATIC <= RS_LDS_MAX,
              "a band of one row fits whatever the shape");
bool vh_resample_plan(const vh_batch *b, const int64_t src_shape[3], const int32_t *h_tab, RsPlan &p) {
    if (b->nb > 65535) return false;   // (grid y)
    const int R = (int)b->R, C = (int)b->C, Z = (int)b->Z;
    p.Rs = (int)src_shape[0]; p.Cs = (int)src_shape[1]; p.Zs = (int)src_shape[2];
    p.ntz = (Z + RS_TZ - 1) / RS_TZ;
    p.TZ = (Z + p.ntz - 1) / p.ntz;
    const int tcmax = std::min(RS_TC, std::max(1, RS_TILE / p.TZ));
    p.ntc = (C + tcmax - 1) / tcmax;
    p.TC = (C + p.ntc - 1) / p.ntc;
    size_t budget = RS_LDS_DEFAULT;
    if (const char *e = getenv("VH_RS_LDS_KB")) budget = (size_t)std::min(64, std::max(1, atoi(e))) * 1024;
    const int64_t stride = 10 * ((int64_t)R + C + Z);
    // the most taps of a column and of a slice anywhere in the batch: what picks the kernel's form
    p.kc = p.kz = 0;
    for (int64_t q = 0; q < b->nb; ++q) {
        const int32_t *cc = h_tab + q * stride + 10 * (int64_t)R + C, *cz = h_tab + q * stride + 10 * ((int64_t)R + C) + Z;
        for (int c = 0; c < C; ++c) p.kc = std::max(p.kc, (int)cc[c]);
        for (int z = 0; z < Z; ++z) p.kz = std::max(p.kz, (int)cz[z]);
    }
    p.BR = 0;
    for (int br = std::min(R, RS_BAND); br >= 1; --br) {
        int span = 0;
        for (int64_t q = 0; q < b->nb; ++q) {
            const int32_t *first = h_tab + q * stride, *count = first + R;
            for (int r0 = 0; r0 < R; r0 += br) {
                int base = INT_MAX, end = 0;
                for (int r = r0; r < std::min(R, r0 + br); ++r)
                    if (count[r] > 0) {
                        base = std::min(base, first[r]);
                        end = std::max(end, first[r] + count[r]);
                    }
                if (end > base) span = std::max(span, end - base);
            }
        }
        span = std::max(span, 1);
        if (rs_lds_bytes(span, p.TC, p.TZ) <= budget || br == 1) {
            p.BR = br;
            p.span = span;
            break;
        }
    }
    // (a tap table has at most 8 taps per index, so span <= 8 at one row: the assertion above holds the
    // launch inside RS_LDS_MAX; bands x tiles is at most R C Z, below 2^31 for every batch)
    p.nbands = (R + p.BR - 1) / p.BR;
    return rs_lds_bytes(p.span, p.TC, p.TZ) <= RS_LDS_MAX;
}

void vh_resample_launch(vh_batch *b, const RsPlan &p, const float *src, float *dst, const int32_t *d_tab) {
    const dim3 grid((unsigned)(p.nbands * p.ntc * p.ntz), (unsigned)b->nb, 1);
    // stamped: the kernel follows the tables' upload on the stream (see vh_mask_paint_launch)
    ScopedKTimer tm(b, "resample_b", 4.0 * (double)b->nb * ((double)p.Rs * p.Cs * p.Zs + (double)b->V), true);
    const size_t lds = rs_lds_dynamic(p.span, p.TC, p.TZ);
    const int R = (int)b->R, C = (int)b->C, Z = (int)b->Z;
    // the form: the smallest of 2, 4, 8 c-taps and of 1, 2 z-taps that covers the batch's tables; more than
    // two z-taps anywhere (a slice scale above 1, or below it off the grid) take the general form
    void (*k)(const float *, float *, const int32_t *, int, int, int, RsPlan, unsigned long long *);
    if (p.kz > 2)
        k = k_resample_b<0, 1>;
    else if (p.kz == 2)
        k = p.kc <= 2 ? k_resample_b<2, 2> : p.kc <= 4 ? k_resample_b<4, 2> : k_resample_b<8, 2>;
    else
        k = p.kc <= 2 ? k_resample_b<2, 1> : p.kc <= 4 ? k_resample_b<4, 1> : k_resample_b<8, 1>;
    k<<<grid, RS_TPB, lds, b->stream>>>(src, dst, d_tab, R, C, Z, p, tm.stamp());
    VH_CHECK_LAUNCH();
}
