// register_maps.hip -- the fine registration of a resident batch (vh_batch_register_maps): the joint
// histogram of the resident HPvent and the resident source proton resampled through every candidate map
// of a grid (scale x sub-voxel offset per axis); the spec is in include/vent_hip.h.  One fused kernel:
// the z- and c-passes of resample.hip into LDS, shared by the r candidates, then per wave the r-pass of
// one candidate, its codes and its counts as register.hip's k_reg_joint keeps them.  No resampled volume
// is ever written.  Every count is an exact integer and every value the bits vh_batch_resample_proton
// would write; the scores come from register.hip's k_reg_score.
#include <algorithm>
#include <climits>

#include "vh_internal.h"

#define RM_TPB 256                  // the code pass
#define RM_NW 8                     // waves of a workgroup: an r candidate (or a share of its rows) each
#define RM_NC 2                     // copies of a wave's histogram: lane l counts in copy l % RM_NC
#define RM_HP 1025                  // words between the copies: the copies of a bin lie on different banks
#define RM_JTPB (64 * RM_NW)
#define RM_TAPS VH_RESAMPLE_TAPS
#define RM_WP (RM_TAPS + 1)         // words between the weights of neighbouring indices in LDS, as RS_WP
#define RM_PAIRS 512                // destination (column, slice) pairs of a tile at most
#define RM_TZ 64                    // slices of a tile at most
#define RM_BAND 32                  // destination rows of a band at most
#define RM_LDS_MAX (156 * 1024)     // histograms, slab, codes and tables: inside the CU's 160 KiB
#define RM_LDS_PLAIN (64 * 1024)    // above it the launch needs MaxDynamicSharedMemorySize
#define RM_HIST_WORDS (RM_NW * RM_NC * RM_HP)
#define RM_ROWS 4                   // source rows whose reads the slab pass has in flight together

// ---- the xenon codes ------------------------------------------------------------------------------
// cx [nb][V] = the codes of the HPvent by its own maximum (maxb [2][nb]: source, HPvent), as k_reg_codes
// writes them; a study whose source or xenon maximum is not > 0 is unregistrable: its codes are never
// read, and are written as invalid.  grid (blocks, nb)
__global__ void __launch_bounds__(RM_TPB) k_rm_codes(const float *__restrict__ x, int64_t V,
                                                     const uint32_t *__restrict__ maxb, int64_t nb,
                                                     uint8_t *__restrict__ cx) {
    const float sm = __uint_as_float(maxb[blockIdx.y]), xm = __uint_as_float(maxb[nb + blockIdx.y]);
    const bool ok = sm > 0.0f && xm > 0.0f;
    const float xs = __fdiv_rn(256.0f, xm);
    const int64_t base = (int64_t)blockIdx.y * V;
    const int64_t step = (int64_t)gridDim.x * RM_TPB;
    for (int64_t i = blockIdx.x * (int64_t)RM_TPB + threadIdx.x; i < V; i += step)
        cx[base + i] = (uint8_t)(ok ? rg_code(x[base + i], xs) : RG_INVALID);
}

// ---- the fused kernel -----------------------------------------------------------------------------
// One workgroup = one study, one (kz, kc), one tile (a band of BR destination rows, TC columns, TZ
// slices) and one chunk of the r list: grid (bands x column tiles x slice tiles, Kz x Kc x chunks, nb).
// LDS: the waves' histograms; the slab [span][TC TZ] floats; the c- and z-table of the tile (weights at
// pitch RM_WP, first, count); the xenon codes of the tile [BR][TC TZ] bytes.
//   1. the slab: row jl holds, for every (c, z) of the tile, the c-sum of source row base + jl under the
//      c map kc and the z map kz, base .. end - 1 the union of the source rows the band's rows tap under
//      the chunk's r candidates (the host sized span from the same tables).  Built once.
//   2. the xenon codes of the tile, invalid where the column or the slice has no tap: such a voxel looks
//      outside the source and is not counted (the spec's skip rule; a row with no tap is skipped whole).
//   3. wave w takes items w, w + RM_NW, ...: an item is an r candidate of the chunk, or, where the chunk
//      has fewer candidates than the workgroup waves, one of nsplit interleaved shares of the band's rows
//      under one.  Per destination row the taps are uniform in the wave; a lane runs the r-pass of its
//      (c, z) pairs from the slab with separately rounded multiplies and adds, codes the value by the
//      study's one scale and counts the pair with the xenon code in its wave's own histogram -- RM_NC
//      copies, bin (0, 0) in a register, exactly as k_reg_joint.  After the item the wave adds its
//      occupied bins to the candidate's global histogram (zeroed by the caller) and clears them.
__global__ void __launch_bounds__(RM_JTPB) k_register_maps(const float *__restrict__ src, const uint8_t *__restrict__ cx,
                                                           const int32_t *__restrict__ tab,
                                                           const uint32_t *__restrict__ maxb, int64_t nb, RmPlan p,
                                                           uint32_t *__restrict__ hist, unsigned long long *ks) {
    extern __shared__ uint32_t s_rm[];
    __shared__ int s_be[2];   // base, end
    kst_begin(ks);
    const float sm = __uint_as_float(maxb[blockIdx.z]), xm = __uint_as_float(maxb[nb + blockIdx.z]);
    if (sm > 0.0f && xm > 0.0f) {   // (the whole workgroup: the maxima are per study)
        const int tid = threadIdx.x, lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: the row taps go through scalar registers)
        const int R = p.R, C = p.C, Z = p.Z;
        const int pe = p.TC * p.TZ;
        uint32_t *s_h = s_rm + wave * (RM_NC * RM_HP);
        uint32_t *mine = s_h + (lane % RM_NC) * RM_HP;
        float *s_slab = reinterpret_cast<float *>(s_rm + RM_HIST_WORDS);
        float *s_wc = s_slab + (size_t)p.span * pe;
        float *s_wz = s_wc + RM_WP * p.TC;
        int32_t *s_fc = reinterpret_cast<int32_t *>(s_wz + RM_WP * p.TZ);
        int32_t *s_kc = s_fc + p.TC;
        int32_t *s_fz = s_kc + p.TC;
        int32_t *s_kz = s_fz + p.TZ;
        uint8_t *s_x = reinterpret_cast<uint8_t *>(s_kz + p.TZ);

        int t = (int)blockIdx.x;
        const int tz = t % p.ntz; t /= p.ntz;
        const int tc = t % p.ntc;
        const int band = t / p.ntc;
        int y = (int)blockIdx.y;
        const int ch = y % p.nchunks; y /= p.nchunks;
        const int kci = y % p.Kc, kzi = y / p.Kc;
        const int r0 = band * p.BR, nr = min(p.BR, R - r0);
        const int c0 = tc * p.TC, ncol = min(p.TC, C - c0);
        const int z0 = tz * p.TZ, nz = min(p.TZ, Z - z0);
        const int ne = ncol * nz;
        const int ka = ch * p.chunk, nk = min(p.chunk, p.Kr - ka);

        // the study's tables: Kr of R, Kc of C, Kz of Z indices, each first [n], count [n], weight [n][8]
        const int32_t *tr = tab + (int64_t)blockIdx.z * 10 * ((int64_t)p.Kr * R + (int64_t)p.Kc * C + (int64_t)p.Kz * Z);
        const int32_t *tcx = tr + 10 * (int64_t)p.Kr * R + 10 * (int64_t)kci * C;
        const int32_t *tzx = tr + 10 * ((int64_t)p.Kr * R + (int64_t)p.Kc * C) + 10 * (int64_t)kzi * Z;
        const float *wc = reinterpret_cast<const float *>(tcx + 2 * (int64_t)C);
        const float *wz = reinterpret_cast<const float *>(tzx + 2 * (int64_t)Z);

        for (int i = tid; i < RM_HIST_WORDS; i += RM_JTPB) s_rm[i] = 0u;
        if (tid == 0) { s_be[0] = INT_MAX; s_be[1] = 0; }
        for (int i = tid; i < ncol; i += RM_JTPB) { s_fc[i] = tcx[c0 + i]; s_kc[i] = tcx[C + c0 + i]; }
        for (int i = tid; i < nz; i += RM_JTPB) { s_fz[i] = tzx[z0 + i]; s_kz[i] = tzx[Z + z0 + i]; }
        for (int i = tid; i < ncol * RM_TAPS; i += RM_JTPB)
            s_wc[(i / RM_TAPS) * RM_WP + i % RM_TAPS] = wc[(int64_t)c0 * RM_TAPS + i];
        for (int i = tid; i < nz * RM_TAPS; i += RM_JTPB)
            s_wz[(i / RM_TAPS) * RM_WP + i % RM_TAPS] = wz[(int64_t)z0 * RM_TAPS + i];
        __syncthreads();

        // the source rows of the band under the chunk's r candidates
        for (int i = tid; i < nk * nr; i += RM_JTPB) {
            const int32_t *trk = tr + 10 * (int64_t)(ka + i / nr) * R;
            const int r = r0 + i % nr;
            const int k = trk[R + r];
            if (k > 0) {
                const int f = trk[r];
                atomicMin(&s_be[0], f);
                atomicMax(&s_be[1], f + k);
            }
        }
        // the xenon codes of the tile; a pair with no c- or z-tap is not counted
        const uint8_t *gx = cx + (int64_t)blockIdx.z * R * C * Z;
        for (int i = tid; i < nr * ne; i += RM_JTPB) {
            const int rl = i / ne, e = i - rl * ne;
            const int cl = e / nz, zl = e - cl * nz;
            const bool in = s_kc[cl] > 0 && s_kz[zl] > 0;
            s_x[rl * pe + e] = in ? gx[((int64_t)(r0 + rl) * C + c0 + cl) * Z + z0 + zl] : (uint8_t)RG_INVALID;
        }
        __syncthreads();
        int base = s_be[0];
        const int end = s_be[1];
        const int rows = end > base ? min(end - base, p.span) : 0;
        if (rows == 0) base = 0;

        // z- and c-pass, as k_resample_b's general form.  The taps of a table lie inside the source, so
        // every read does
        const float *S = src + (int64_t)blockIdx.z * p.Rs * p.Cs * p.Zs;
        for (int e = tid; e < ne; e += RM_JTPB) {
            const int cl = e / nz, zl = e - cl * nz;
            const int fc = s_fc[cl], kc = s_kc[cl], fz = s_fz[zl], kz = s_kz[zl];
            const float *wcl = s_wc + cl * RM_WP, *wzl = s_wz + zl * RM_WP;
            const float *at = S + ((int64_t)base * p.Cs + fc) * p.Zs + fz;
            const int64_t rp = (int64_t)p.Cs * p.Zs;
            // RM_ROWS source rows at a time, so that as many reads are in flight (a row past the last
            // re-reads the last and is not stored); every row's sums are its own, in the spec's order
            for (int jl = 0; jl < rows; jl += RM_ROWS) {
                const float *row[RM_ROWS];
                float ac[RM_ROWS];
#pragma unroll
                for (int u = 0; u < RM_ROWS; ++u) {
                    row[u] = at + (int64_t)min(jl + u, rows - 1) * rp;
                    ac[u] = 0.0f;
                }
                for (int a = 0; a < kc; ++a) {
                    float az[RM_ROWS];
#pragma unroll
                    for (int u = 0; u < RM_ROWS; ++u) az[u] = 0.0f;
                    for (int k = 0; k < kz; ++k) {
                        const float w = wzl[k];
                        float v[RM_ROWS];
#pragma unroll
                        for (int u = 0; u < RM_ROWS; ++u) v[u] = row[u][(int64_t)a * p.Zs + k];
#pragma unroll
                        for (int u = 0; u < RM_ROWS; ++u) az[u] = __fadd_rn(az[u], __fmul_rn(w, v[u]));
                    }
                    const float w = wcl[a];
#pragma unroll
                    for (int u = 0; u < RM_ROWS; ++u) ac[u] = __fadd_rn(ac[u], __fmul_rn(w, az[u]));
                }
#pragma unroll
                for (int u = 0; u < RM_ROWS; ++u)
                    if (jl + u < rows) s_slab[(jl + u) * pe + e] = ac[u];
            }
        }
        __syncthreads();

        // r-pass and counts (no barrier below: a wave's histogram is its own)
        const float scale = __fdiv_rn(256.0f, sm);
        const int nsplit = max(1, RM_NW / nk);
        const size_t nc = (size_t)p.Kr * p.Kc * p.Kz;
        uint32_t *hs = hist + (size_t)blockIdx.z * nc * RG_BINS;
        for (int it = wave; it < nk * nsplit; it += RM_NW) {
            const int kri = ka + it / nsplit, part = it % nsplit;
            const int32_t *trk = tr + 10 * (int64_t)kri * R;
            const float *wrk = reinterpret_cast<const float *>(trk + 2 * (int64_t)R);
            uint32_t n00 = 0u;
            for (int rl = part; rl < nr; rl += nsplit) {
                const int r = r0 + rl;
                const int f = trk[r], k = trk[R + r];
                // (a row with no tap is skipped; the second test never holds: the slab covers every tap)
                if (k <= 0 || f < base || f - base + k > rows) continue;
                float w[RM_TAPS];
#pragma unroll
                for (int a = 0; a < RM_TAPS; ++a) w[a] = wrk[(int64_t)r * RM_TAPS + a];
                const float *st = s_slab + (f - base) * pe;
                const uint8_t *xr = s_x + rl * pe;
                for (int e = lane; e < ne; e += 64) {
                    const uint32_t b = xr[e];
                    float ar = 0.0f;
#pragma unroll
                    for (int a = 0; a < RM_TAPS; ++a)
                        if (a < k) ar = __fadd_rn(ar, __fmul_rn(w[a], st[a * pe + e]));
                    const uint32_t a32 = rg_code(ar, scale);
                    // t: 0 for a pair of bin (0, 0), 1..31 for any other valid pair, above for an invalid one
                    const uint32_t tt = a32 | b;
                    if (tt == 0u) ++n00;
                    else if (tt < 32u) atomicAdd(mine + (a32 << 5) + b, 1u);
                }
            }
            for (int off = 32; off > 0; off >>= 1) n00 += __shfl_xor(n00, off, 64);
            // (a wave's LDS operations complete in program order: the adds above precede these reads)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t *out = hs + ((size_t)(kzi * p.Kr + kri) * p.Kc + kci) * RG_BINS;
#pragma unroll 4
            for (int k = lane; k < RG_BINS; k += 64) {
                uint32_t n = k == 0 ? n00 : 0u;
#pragma unroll
                for (int c = 0; c < RM_NC; ++c) {
                    const uint32_t v = s_h[c * RM_HP + k];
                    if (v) s_h[c * RM_HP + k] = 0u;
                    n += v;
                }
                if (n) atomicAdd(out + k, n);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
    kst_end(ks);
}

// LDS of a workgroup beside the static s_be
static size_t rm_lds_bytes(int span, int TC, int TZ, int BR) {
    const size_t pe = (size_t)TC * TZ;
    return sizeof(uint32_t) * ((size_t)RM_HIST_WORDS + (size_t)span * pe + (size_t)(RM_WP + 2) * (TC + TZ)) +
           (((size_t)BR * pe + 3) & ~(size_t)3);
}

// The largest number of source rows a band of br destination rows taps under a chunk of the r list, over
// every study, band and chunk: what k_register_maps finds per workgroup, so what the slab must hold
static int rm_span(const vh_batch *b, const int32_t *h_tab, int Kr, int64_t stride, int br, int chunk) {
    const int R = (int)b->R;
    int span = 1;
    for (int64_t q = 0; q < b->nb; ++q)
        for (int ka = 0; ka < Kr; ka += chunk)
            for (int r0 = 0; r0 < R; r0 += br) {
                int base = INT_MAX, end = 0;
                for (int k = ka; k < std::min(Kr, ka + chunk); ++k) {
                    const int32_t *first = h_tab + q * stride + 10 * (int64_t)k * R, *count = first + R;
                    for (int r = r0; r < std::min(R, r0 + br); ++r)
                        if (count[r] > 0) {
                            base = std::min(base, first[r]);
                            end = std::max(end, first[r] + count[r]);
                        }
                }
                if (end > base) span = std::max(span, end - base);
            }
    return span;
}

// The tile: slices in equal chunks of at most RM_TZ, columns in equal chunks so that a tile has at most
// RM_PAIRS pairs.  The band and the chunk: the whole r list and the most rows, up to RM_BAND (halved down
// to 1), whose slab fits beside the histograms; where not even one row does, the r list is halved until
// it fits.  One row under one candidate always fits: its slab is at most 8 source rows, 16 KiB at
// RM_PAIRS pairs, and the tables of the widest tile take 11 words per column and per slice.
// (VH_RM_LDS_KB, 1..156, is a diagnostics variable like VH_RS_LDS_KB: it sets the KiB that slab, codes
// and tables may take, for the test of the band and chunk logic; no result depends on it, and a budget
// that one row under one candidate does not fit is refused.)
static_assert(sizeof(uint32_t) * (RM_HIST_WORDS + RM_TAPS * RM_PAIRS + (RM_WP + 2) * (RM_PAIRS + RM_TZ)) + RM_PAIRS <=
                  RM_LDS_MAX,
              "one row under one candidate fits whatever the shape");
bool vh_register_maps_plan(const vh_batch *b, const int64_t src_shape[3], const int32_t count[3],
                           const int32_t *h_tab, RmPlan &p) {
    if (b->nb > 65535 || b->R * b->C * b->Z >= ((int64_t)1 << 31)) return false;   // (grid z, grid x)
    const int R = (int)b->R, C = (int)b->C, Z = (int)b->Z;
    p.Rs = (int)src_shape[0]; p.Cs = (int)src_shape[1]; p.Zs = (int)src_shape[2];
    p.R = R; p.C = C; p.Z = Z;
    p.Kr = count[0]; p.Kc = count[1]; p.Kz = count[2];
    p.ntz = (Z + RM_TZ - 1) / RM_TZ;
    p.TZ = (Z + p.ntz - 1) / p.ntz;
    const int tcmax = std::max(1, RM_PAIRS / p.TZ);
    p.ntc = (C + tcmax - 1) / tcmax;
    p.TC = (C + p.ntc - 1) / p.ntc;
    size_t budget = RM_LDS_MAX;
    if (const char *e = getenv("VH_RM_LDS_KB"))
        budget = std::min<size_t>(RM_LDS_MAX, sizeof(uint32_t) * RM_HIST_WORDS +
                                                  (size_t)std::min(156, std::max(1, atoi(e))) * 1024);
    const int64_t stride = 10 * ((int64_t)p.Kr * R + (int64_t)p.Kc * C + (int64_t)p.Kz * Z);
    p.BR = 0;
    for (int chunk = p.Kr; p.BR == 0; chunk = (chunk + 1) / 2) {
        for (int br = std::min(R, RM_BAND);; br = (br + 1) / 2) {
            const int span = rm_span(b, h_tab, p.Kr, stride, br, chunk);
            if (rm_lds_bytes(span, p.TC, p.TZ, br) <= budget) {
                p.BR = br; p.span = span; p.chunk = chunk;
                break;
            }
            if (br == 1) break;
        }
        if (chunk == 1) break;
    }
    if (p.BR == 0) return false;   // (under VH_RM_LDS_KB only: see the assertion above)
    p.nbands = (R + p.BR - 1) / p.BR;
    p.nchunks = (p.Kr + p.chunk - 1) / p.chunk;
    return true;
}

void vh_register_maps_launch(vh_batch *b, const RmPlan &p, const float *src, const float *hp, const int32_t *d_tab,
                             uint32_t *d_maxb, uint8_t *d_cx, uint32_t *d_hist, double *d_score) {
    const size_t nb = (size_t)b->nb;
    const int nc = p.Kr * p.Kc * p.Kz;
    const size_t lds = rm_lds_bytes(p.span, p.TC, p.TZ, p.BR);
    if (lds > RM_LDS_MAX) throw VhError{VH_ERR_ARG, "register_maps: the tile does not fit"};
    HIP_TRY(hipMemsetAsync(d_maxb, 0, sizeof(uint32_t) * 2 * nb, b->stream));
    vh_seg_max_launch_n(b, src, (int64_t)p.Rs * p.Cs * p.Zs, d_maxb);
    vh_seg_max_launch(b, hp, d_maxb + nb);
    {
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((b->V + RM_TPB * 8 - 1) / (RM_TPB * 8), 256));
        ScopedKTimer tm(b, "register_maps_codes_b", 5.0 * (double)nb * (double)b->V);
        k_rm_codes<<<dim3((unsigned)blocks, (unsigned)nb, 1), RM_TPB, 0, b->stream>>>(hp, b->V, d_maxb, b->nb, d_cx);
        VH_CHECK_LAUNCH();
    }
    HIP_TRY(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * nb * (size_t)nc * RG_BINS, b->stream));
    {
        if (lds > RM_LDS_PLAIN) vh_set_max_lds((const void *)k_register_maps, RM_LDS_MAX);
        const dim3 grid((unsigned)(p.nbands * p.ntc * p.ntz), (unsigned)(p.Kz * p.Kc * p.nchunks), (unsigned)nb);
        // stamped: the kernel follows the tables' upload on the stream (see vh_mask_paint_launch)
        ScopedKTimer tm(b, "register_maps_b",
                        (double)nb * (4.0 * (double)p.Rs * p.Cs * p.Zs + (double)b->V) * (double)(p.Kz * p.Kc), true);
        k_register_maps<<<grid, RM_JTPB, lds, b->stream>>>(src, d_cx, d_tab, d_maxb, b->nb, p, d_hist, tm.stamp());
        VH_CHECK_LAUNCH();
    }
    vh_register_score_launch(b, d_hist, d_maxb, nc, d_score);
}
