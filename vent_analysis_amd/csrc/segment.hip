// segment.hip -- the lungs from the proton image of a resident batch: the statistics sweep behind the
// Otsu threshold (vh_batch_proton_threshold), the border-seeded flood fill (vh_batch_segment) and the
// overlap counts against another mask (vh_batch_mask_overlap); the spec is in include/vent_hip.h.
// Every step is a max, an integer count or bit logic.
#include <algorithm>

#include "vh_internal.h"

#define SG_TPB 256
#define SG_FTPB 256             // the fill (1024 threads: the same time at 32 slices per field, 1.4 - 1.8 x at 16 and 8)
#define SG_LDS_MAX (156 * 1024)   // both bit sets of a plane: inside the CU's 160 KiB
#define SG_LDS_PLAIN (64 * 1024)  // above it the launch needs MaxDynamicSharedMemorySize

// ---- statistics -----------------------------------------------------------------------------------
// in F: finite and >= 0 (NaN fails both comparisons; -0.0 is in F and counts as +0.0)
__device__ __forceinline__ bool sg_in_f(float x) { return x >= 0.0f && x <= 3.402823466e+38f; }

// f(x) for every voxel of a study, this thread's share of the grid's: float4 loads between the first
// and the last 16-byte boundary (a study starts at any float), the few floats before and after one by one
template <class F>
__device__ __forceinline__ void sg_for_each(const float *__restrict__ xs, int64_t V, F f) {
    const int64_t lead = (int64_t)(((16u - (uint32_t)((uintptr_t)xs & 15u)) & 15u) >> 2);
    const int64_t head = lead < V ? lead : V;
    const int64_t n4 = (V - head) >> 2, tail0 = head + (n4 << 2);
    const int64_t t = blockIdx.x * (int64_t)SG_TPB + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * SG_TPB;
    const float4 *x4 = reinterpret_cast<const float4 *>(xs + head);
#pragma unroll 4
    for (int64_t i = t; i < n4; i += step) {
        const float4 v = x4[i];
        f(v.x); f(v.y); f(v.z); f(v.w);
    }
    if (t < head) f(xs[t]);
    if (tail0 + t < V) f(xs[tail0 + t]);
}

// pmax_bits[study] = max over F of the bit pattern (non-negative floats order as their bits; zeroed by
// the caller, so an empty F leaves +0.0): grid (chunks, nb)
__global__ void __launch_bounds__(SG_TPB) k_seg_max(const float *__restrict__ x, int64_t V, uint32_t *pmax_bits,
                                                    unsigned long long *ks) {
    kst_begin(ks);
    uint32_t m = 0u;
    sg_for_each(x + (int64_t)blockIdx.y * V, V, [&](float v) {
        if (sg_in_f(v)) m = max(m, __float_as_uint(v) & 0x7fffffffu);
    });
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(pmax_bits + blockIdx.y, m);
    kst_end(ks);
}

// hist[study][256] += the counts of F in bin min(255, (int)(x * scale)), scale = 256.0f / pmax (zeroed
// by the caller; untouched when pmax is not > 0): LDS counters per workgroup -- SG_HC copies of each
// bin, a thread counting in copy tid % SG_HC, as an image puts most of a wave into a few bins and
// adds to one LDS word go one after the other; copy j starts at word 257 j, so the copies of a bin lie
// on different banks -- then one add per occupied bin.  A product that is not below 255 (an infinite
// scale included) counts in bin 255.
#define SG_HC 8
#define SG_HP 257
__global__ void __launch_bounds__(SG_TPB) k_seg_hist(const float *__restrict__ x, int64_t V,
                                                     const uint32_t *__restrict__ pmax_bits, uint32_t *hist,
                                                     unsigned long long *ks) {
    __shared__ uint32_t s_h[SG_HP * SG_HC];
    kst_begin(ks);
    const float pmax = __uint_as_float(pmax_bits[blockIdx.y]);
    if (pmax > 0.0f) {   // (the whole workgroup: pmax is per study)
        const float scale = __fdiv_rn(256.0f, pmax);
#pragma unroll
        for (int j = 0; j < SG_HC; ++j) s_h[j * SG_HP + threadIdx.x] = 0u;
        __syncthreads();
        uint32_t *mine = s_h + (threadIdx.x & (SG_HC - 1)) * SG_HP;
        sg_for_each(x + (int64_t)blockIdx.y * V, V, [&](float v) {
            if (sg_in_f(v)) {
                const float p = __fmul_rn(v, scale);
                atomicAdd(mine + (p < 255.0f ? (int)p : 255), 1u);
            }
        });
        __syncthreads();
        uint32_t n = 0u;
#pragma unroll
        for (int j = 0; j < SG_HC; ++j) n += s_h[j * SG_HP + threadIdx.x];
        if (n) atomicAdd(hist + (int64_t)blockIdx.y * 256 + threadIdx.x, n);
    }
    kst_end(ks);
}

// the maximum sweep alone (d_max_bits zeroed by the caller): the registration takes it for both images
void vh_seg_max_launch_n(vh_batch *b, const float *x, int64_t n, uint32_t *d_max_bits) {
    if (b->nb > 65535) throw VhError{VH_ERR_ARG, "more than 65535 studies"};   // (grid y)
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((n + SG_TPB * 128 - 1) / (SG_TPB * 128), 32));
    ScopedKTimer tm(b, "segment_max_b", 4.0 * (double)b->nb * (double)n, true);
    k_seg_max<<<dim3((unsigned)chunks, (unsigned)b->nb, 1), SG_TPB, 0, b->stream>>>(x, n, d_max_bits, tm.stamp());
    VH_CHECK_LAUNCH();
}
void vh_seg_max_launch(vh_batch *b, const float *x, uint32_t *d_max_bits) { vh_seg_max_launch_n(b, x, b->V, d_max_bits); }

void vh_proton_stats_launch(vh_batch *b, const float *proton, uint32_t *d_pmax_bits, uint32_t *d_hist) {
    static_assert(SG_TPB == 256, "one thread per histogram bin");
    const size_t nb = (size_t)b->nb;
    if (b->nb > 65535) throw VhError{VH_ERR_ARG, "proton_threshold: more than 65535 studies"};   // (grid y)
    HIP_TRY(hipMemsetAsync(d_pmax_bits, 0, sizeof(uint32_t) * nb, b->stream));
    HIP_TRY(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * 256 * nb, b->stream));
    // 32 float4 loads per thread: with 4 (96 workgroups per study of the bench batch) the two sweeps took
    // 0.38 + 0.31 ms, workgroups ending as soon as they had started
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((b->V + SG_TPB * 128 - 1) / (SG_TPB * 128), 32));
    const dim3 grid((unsigned)chunks, (unsigned)b->nb, 1);
    vh_seg_max_launch(b, proton, d_pmax_bits);
    ScopedKTimer tm(b, "segment_hist_b", 4.0 * (double)b->nb * (double)b->V, true);
    k_seg_hist<<<grid, SG_TPB, 0, b->stream>>>(proton, b->V, d_pmax_bits, d_hist, tm.stamp());
    VH_CHECK_LAUNCH();
}

// ---- the fill -------------------------------------------------------------------------------------
struct SgGeom {
    int R, C, Z;
    int ZC;          // slices per chunk: 1, 2, 4, 8, 16 or 32 bits of a pixel's field
    int lz;          // log2(ZC)
    int wpr, pitch;  // words that hold a row's C fields (32 / ZC fields each); the odd row pitch in words
    int nzc;         // slice chunks (blockIdx.x)
};

// a nibble (bit j = slice j) as four 0 / 1 bytes: the product's partial terms fall on distinct bits
__device__ __forceinline__ uint32_t sg_unnib(uint32_t n) { return ((n & 0xfu) * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ uint32_t sg_nz01(uint32_t x) {   // the bytes of a word that are not 0, as 0 / 1
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
}

// One directional pass along a line of n words (word k of the line at k * stride; DIR -1 walks it from
// its end): reach |= dark & reach(previous field), fields of zc bits.  Inside a word the run is closed by
// an occluded fill in log2(32 / zc) shifts; the last field of a word is carried into the next.  Four
// words are read ahead of the chain, so an LDS read's latency is paid once per four steps; a word is
// written only where it changed.  Returns whether any did.
template <int DIR>
__device__ __forceinline__ int sg_pass(const uint32_t *dd, uint32_t *rr, int n, int stride, int zc) {
    int changed = 0;
    uint32_t carry = 0u;
    for (int k0 = 0; k0 < n; k0 += 4) {
        uint32_t d[4], r0[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < n;
            const int at = (DIR > 0 ? k0 + j : n - 1 - k0 - j) * stride;
            d[j] = in ? dd[at] : 0u;       // (past the end: not dark, so nothing is written)
            r0[j] = in ? rr[at] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t gen = r0[j] | (d[j] & carry), pro = d[j];
            for (int s = zc; s < 32; s <<= 1) {
                gen |= pro & (DIR > 0 ? gen << s : gen >> s);
                pro &= DIR > 0 ? pro << s : pro >> s;
            }
            if (gen != r0[j]) {
                rr[(DIR > 0 ? k0 + j : n - 1 - k0 - j) * stride] = gen;
                changed = 1;
            }
            carry = DIR > 0 ? gen >> (32 - zc) : gen << (32 - zc);
        }
    }
    return changed;
}

// One workgroup = one (study, chunk of ZC slices): grid (nzc, nb).
//
// The slice axis is fastest in memory, so the ZC slices of a pixel pack into one ZC-bit field (bit z =
// slice z0 + z) and 32 / ZC fields into a word: pixel (r, c) is field c % (32 / ZC) of word
// r * pitch + c / (32 / ZC).  Two such bit sets of the whole plane live in LDS: s_d (dark = x < t) and
// s_r (reach).  Every AND / OR advances all slices of the chunk, and 32 / ZC pixels, at once.  Fields
// past column C - 1 and slices past Z - 1 are never dark, so nothing reaches or leaves them.
//
// Packing, any shape (WORD false): lane = (pixel p, slice z) of 64 / ZC pixels, so a wave loads
// consecutive floats; __ballot packs the comparisons and lane p takes its pixel's field.  When Z is a
// multiple of 4 and ZC at least 4 (WORD true: a pixel's slices of the chunk are aligned float4s) a
// thread loads its pixel's quads.  Fields enter LDS by an OR, as several pixels share a word.
//
// The fill: reach = dark on rows 0 and R - 1 and columns 0 and C - 1; then rounds of four directional
// sweeps, each reach |= dark & reach(previous pixel) (sg_pass): along the rows one thread per row,
// along the columns one thread per word column.  The pitch is odd, so the 32 rows of a half wave fall
// on 32 banks.  A round that changes nothing ends the loop -- the vote is __syncthreads_or, uniform --
// and the loop is bounded by R * C rounds, which always suffice (a round that is not the last adds a
// pixel), whatever the input.  seg = dark & ~reach leaves as 0 / 1 bytes: whole 32-bit words of
// consecutive addresses (WORD), else consecutive bytes.
template <bool WORD>
__global__ void __launch_bounds__(SG_FTPB) k_seg_fill(const float *__restrict__ x, uint8_t *__restrict__ seg,
                                                     const float *__restrict__ thresh, int64_t V, SgGeom g,
                                                     unsigned long long *ks) {
    extern __shared__ uint32_t s_sg[];
    kst_begin(ks);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = g.R, C = g.C, ZC = g.ZC, lz = g.lz, pitch = g.pitch, wpr = g.wpr;
    const int lp = 5 - lz;                 // log2(fields per word)
    const int fm = (1 << lp) - 1;          // field index mask
    const int RC = R * C;
    const int z0 = (int)blockIdx.x * ZC;
    const int nz = min(ZC, g.Z - z0);
    const uint32_t zmask = nz >= 32 ? 0xffffffffu : (1u << nz) - 1u;
    const float t = thresh[blockIdx.y];
    const float *xs = x + (int64_t)blockIdx.y * V;
    uint8_t *ys = seg + (int64_t)blockIdx.y * V;
    uint32_t *s_d = s_sg, *s_r = s_sg + R * pitch;

    for (int i = tid; i < R * pitch; i += SG_FTPB) s_d[i] = 0u;
    __syncthreads();
    if (WORD) {
        const int nq = nz >> 2;
        for (int pix = tid; pix < RC; pix += SG_FTPB) {
            const float4 *px = reinterpret_cast<const float4 *>(xs + (int64_t)pix * g.Z + z0);
            uint32_t f = 0u;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < nq) {
                    const float4 v = px[q];
                    f |= ((uint32_t)(v.x < t) | (uint32_t)(v.y < t) << 1 | (uint32_t)(v.z < t) << 2 |
                          (uint32_t)(v.w < t) << 3) << (4 * q);
                }
            const int r = pix / C, c = pix - r * C;
            if (f) atomicOr(&s_d[r * pitch + (c >> lp)], f << ((c & fm) << lz));
        }
    } else {
        const int P = 64 >> lz;            // pixels per wave load
        const int p = lane >> lz, z = lane & (ZC - 1);
        for (int pix0 = wave * P; pix0 < RC; pix0 += (SG_FTPB / 64) * P) {   // (wave-uniform: every lane reaches the ballot)
            const int pix = pix0 + p;
            bool dk = false;
            if (pix < RC && z < nz) dk = xs[(int64_t)pix * g.Z + z0 + z] < t;
            const unsigned long long bal = __ballot(dk);
            const int mine = pix0 + lane;  // the pixel whose field this lane takes
            if (lane < P && mine < RC) {
                const uint32_t f = (uint32_t)(bal >> (lane << lz)) & zmask;
                const int r = mine / C, c = mine - r * C;
                if (f) atomicOr(&s_d[r * pitch + (c >> lp)], f << ((c & fm) << lz));
            }
        }
    }
    __syncthreads();

    // the seeds: the dark pixels of the four edges
    {
        const uint32_t f0 = zmask;                                  // column 0: field 0 of word 0
        const int wl = (C - 1) >> lp;
        const uint32_t fl = zmask << (((C - 1) & fm) << lz);        // column C - 1
        for (int i = tid; i < R * pitch; i += SG_FTPB) {
            const int r = i / pitch, w = i - r * pitch;
            uint32_t m = 0u;
            if (r == 0 || r == R - 1) m = 0xffffffffu;
            if (w == 0) m |= f0;
            if (w == wl) m |= fl;
            s_r[i] = s_d[i] & m;
        }
    }
    __syncthreads();

    const int max_rounds = RC;
    for (int round = 0; round < max_rounds; ++round) {
        int changed = 0;
        for (int r = tid; r < R; r += SG_FTPB) {
            changed |= sg_pass<1>(s_d + r * pitch, s_r + r * pitch, wpr, 1, ZC);    // left -> right
            changed |= sg_pass<-1>(s_d + r * pitch, s_r + r * pitch, wpr, 1, ZC);   // right -> left
        }
        __syncthreads();
        for (int w = tid; w < wpr; w += SG_FTPB) {   // a whole word steps to the next row: one field of 32 bits
            changed |= sg_pass<1>(s_d + w, s_r + w, R, pitch, 32);                  // top -> bottom
            changed |= sg_pass<-1>(s_d + w, s_r + w, R, pitch, 32);                 // bottom -> top
        }
        if (!__syncthreads_or(changed)) break;        // (uniform; also the barrier before the next round)
    }

    if (WORD) {
        const int nq = nz >> 2;
        uint32_t *y4 = reinterpret_cast<uint32_t *>(ys);
        for (int d = tid; d < RC * nq; d += SG_FTPB) {
            const int pix = d / nq, q = d - pix * nq;
            const int r = pix / C, c = pix - r * C;
            const int i = r * pitch + (c >> lp);
            const uint32_t f = ((s_d[i] & ~s_r[i]) >> ((c & fm) << lz)) & zmask;
            y4[(((int64_t)pix * g.Z + z0) >> 2) + q] = sg_unnib(f >> (4 * q));
        }
    } else {
        for (int d = tid; d < RC * nz; d += SG_FTPB) {
            const int pix = d / nz, z = d - pix * nz;
            const int r = pix / C, c = pix - r * C;
            const int i = r * pitch + (c >> lp);
            const uint32_t f = (s_d[i] & ~s_r[i]) >> ((c & fm) << lz);
            ys[(int64_t)pix * g.Z + z0 + z] = (uint8_t)((f >> z) & 1u);
        }
    }
    kst_end(ks);
}

static size_t sg_lds_bytes(int R, int C, int ZC) {
    const int wpr = (C * ZC + 31) / 32;
    return 2 * sizeof(uint32_t) * (size_t)R * (size_t)(wpr | 1);
}

// VH_SEG_ZC, read at call time like VH_CI_FORM: 1, 2, 4, 8, 16 or 32 forces the field width where both
// bit sets then fit; otherwise the widest field up to the slice count that fits, so a study takes the
// fewest workgroups and every sweep step carries the most slices
static SgGeom sg_geometry(const vh_batch *b) {
    SgGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    int need = 1;
    while (need < 32 && need < g.Z) need <<= 1;
    int ZC = need;
    while (ZC > 1 && sg_lds_bytes(g.R, g.C, ZC) > SG_LDS_MAX) ZC >>= 1;
    const char *e = getenv("VH_SEG_ZC");
    const int f = e ? atoi(e) : 0;
    if ((f == 1 || f == 2 || f == 4 || f == 8 || f == 16 || f == 32) && sg_lds_bytes(g.R, g.C, f) <= SG_LDS_MAX) ZC = f;
    g.ZC = ZC;
    g.lz = 0;
    while ((1 << g.lz) < ZC) ++g.lz;
    g.wpr = (g.C * ZC + 31) / 32;
    g.pitch = g.wpr | 1;
    g.nzc = (g.Z + ZC - 1) / ZC;
    return g;
}

bool vh_segment_takes(const vh_batch *b) {   // the plane in LDS at one slice per field; grid y
    return b->R <= 512 && b->C <= 512 && b->nb <= 65535 && sg_lds_bytes((int)b->R, (int)b->C, 1) <= SG_LDS_MAX;
}

void vh_segment_launch(vh_batch *b, const float *proton, uint8_t *seg, const float *d_thresh) {
    const SgGeom g = sg_geometry(b);
    const size_t lds = sg_lds_bytes(g.R, g.C, g.ZC);
    if (lds > SG_LDS_MAX) throw VhError{VH_ERR_ARG, "segment: the plane does not fit"};
    // (Z a multiple of 4 makes every pixel's chunk start on a float4 and on a 32-bit word of the mask)
    auto fn = (g.Z % 4 == 0 && g.ZC >= 4) ? k_seg_fill<true> : k_seg_fill<false>;
    if (lds > SG_LDS_PLAIN) vh_set_max_lds((const void *)fn, SG_LDS_MAX);
    const dim3 grid((unsigned)g.nzc, (unsigned)b->nb, 1);
    // stamped: the kernel follows the thresholds' upload on the stream (see vh_mask_paint_launch)
    ScopedKTimer tm(b, "segment_b", 5.0 * (double)b->nb * (double)b->V, true);
    fn<<<grid, SG_FTPB, lds, b->stream>>>(proton, seg, d_thresh, b->V, g, tm.stamp());
    VH_CHECK_LAUNCH();
}

// ---- overlap --------------------------------------------------------------------------------------
// cnt[study][3] += |a != 0|, |o != 0|, |both| (zeroed by the caller): grid (blocks, nb).  a and o are
// [nb][V] from an allocation's start each, so a study starts at the same byte of a 16-byte word in
// both; its bytes up to the first boundary and after the last are read one by one.
__global__ void __launch_bounds__(SG_TPB) k_mask_overlap(const uint8_t *__restrict__ a, const uint8_t *__restrict__ o,
                                                         int64_t V, unsigned long long *cnt) {
    const uint8_t *xa = a + (int64_t)blockIdx.y * V, *xo = o + (int64_t)blockIdx.y * V;
    const int64_t lead = (int64_t)((16u - (uint32_t)((uintptr_t)xa & 15u)) & 15u);
    const int64_t head = lead < V ? lead : V;
    const int64_t n16 = (V - head) >> 4, tail0 = head + (n16 << 4);
    const int64_t t = blockIdx.x * (int64_t)SG_TPB + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * SG_TPB;
    const uint4 *a4 = reinterpret_cast<const uint4 *>(xa + head), *o4 = reinterpret_cast<const uint4 *>(xo + head);
    unsigned long long c[3] = {0, 0, 0};
    for (int64_t i = t; i < n16; i += step) {
        const uint4 m = a4[i], n = o4[i];
        const uint32_t ma[4] = {sg_nz01(m.x), sg_nz01(m.y), sg_nz01(m.z), sg_nz01(m.w)};
        const uint32_t mo[4] = {sg_nz01(n.x), sg_nz01(n.y), sg_nz01(n.z), sg_nz01(n.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[0] += __popc(ma[j]);
            c[1] += __popc(mo[j]);
            c[2] += __popc(ma[j] & mo[j]);
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t at = pass ? tail0 + t : t;
        if (pass ? at < V : at < head) {
            const bool va = xa[at] != 0, vo = xo[at] != 0;
            c[0] += va; c[1] += vo; c[2] += va && vo;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        unsigned long long v = c[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(cnt + (int64_t)blockIdx.y * 3 + j, v);
    }
}

void vh_mask_overlap_launch(vh_batch *b, const uint8_t *a, const uint8_t *o, unsigned long long *d_cnt) {
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((b->V >> 4) + SG_TPB - 1) / SG_TPB, 64));
    for (int64_t y0 = 0; y0 < b->nb; y0 += 65535) {   // (grid y)
        const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(b->nb - y0, 65535), 1);
        k_mask_overlap<<<grid, SG_TPB, 0, b->stream>>>(a + y0 * b->V, o + y0 * b->V, b->V, d_cnt + y0 * 3);
        VH_CHECK_LAUNCH();
    }
}
