// mask_edit.hip -- editing the resident masks of a batch: the per-slice disc morphology
// (vh_batch_edit_mask), the paint strokes (vh_batch_paint_mask) and the voxel count of
// vh_batch_download_mask; the spec is in include/vent_hip.h.  All arithmetic is on bits.
#include <algorithm>

#include "vh_internal.h"

#define ME_TPB 256
#define ME_TR 32             // output rows per workgroup: 8 per wave
#define ME_TC 64             // output columns per workgroup: one per lane
#define ME_SR (ME_TR / (ME_TPB / 64))
#define ME_KMAX 5
#define ME_W (ME_TC + 2 * ME_KMAX)   // words per staged row
#define ME_ZC_MAX 32         // slices per workgroup: one bit each of a pixel's word

struct MeGeom {
    int R, C, Z;
    int ZC;                  // slices per chunk (all of them when Z <= 32)
    int nct, nzc;            // column tiles, slice chunks (blockIdx.x = (row tile * nct + column tile) * nzc + chunk)
};

// half width of the disc's run at row distance d: floor(sqrt(k^2 - d^2))
__host__ __device__ constexpr int me_run(int k, int d) {
    int w = 0;
    while ((w + 1) * (w + 1) + d * d <= k * k) ++w;
    return w;
}

// The dilation of one wave's strip: output rows a .. a + ME_SR - 1 of the tile, column `lane`.  The
// staged tile starts K rows and K columns before the output tile, so output (o, j) is the OR of
// s_x[o + K + dr][j + K + dc] over the disc.  The disc is a union of horizontal runs,
// D_K = U_dr {dr} x [-w(dr), w(dr)]: for a staged row the runs H_w = OR of x(j - w .. j + w) are built
// incrementally, H_w = H_{w-1} | x(j - w) | x(j + w), from 2K + 1 reads (a lane reads consecutive
// words: no bank conflict), and every output row within K of it ORs in the one run its distance
// selects.  Every index below is a compile-time constant after unrolling.
template <int K>
__device__ __forceinline__ void me_dilate_strip(const uint32_t *s_x, int a, int lane, uint32_t (&acc)[ME_SR]) {
#pragma unroll
    for (int ii = 0; ii < ME_SR + 2 * K; ++ii) {
        const uint32_t *row = s_x + (a + ii) * ME_W + lane;
        uint32_t h[K + 1];
        h[0] = row[K];
#pragma unroll
        for (int w = 1; w <= K; ++w) h[w] = h[w - 1] | row[K - w] | row[K + w];
#pragma unroll
        for (int o = 0; o < ME_SR; ++o) {
            const int d = ii - K - o < 0 ? o + K - ii : ii - K - o;
            if (d <= K) acc[o] |= h[me_run(K, d)];
        }
    }
}

// bytes of a 32-bit word that are not 0, as 0 / 1 bytes
__device__ __forceinline__ uint32_t me_nz01(uint32_t x) {
    return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
}
// the four bytes of a word as a nibble (bit j = byte j != 0), and a nibble back as 0 / 1 bytes: the
// products' partial terms fall on distinct bits, so nothing carries
__device__ __forceinline__ uint32_t me_nib(uint32_t x) { return (me_nz01(x) * 0x01020408u) >> 24; }
__device__ __forceinline__ uint32_t me_unnib(uint32_t n) { return ((n & 0xfu) * 0x00204081u) & 0x01010101u; }

// LDS written by one lane of a wave and read by another: program order within the wave is enough
// for the hardware; this keeps the compiler from moving the accesses across it
__device__ __forceinline__ void me_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One launch over the batch: grid (row tiles x column tiles x slice chunks, nb), src -> dst.
//
// The slice axis is fastest in memory, so a pixel's slices pack into one 32-bit word (bit z = slice
// z0 + z != 0) and every OR works on all slices of a pixel at once.  Positions outside the slice, and
// slices past Z - 1 of a ragged last chunk, are 0.  Erosion is the dilation of the complement: the
// words are complemented inside zmask (the chunk's valid slices) as they are staged -- its pad of 1
// is then the same 0 -- and again before the store.  A study of radius 0 is copied byte for byte.
//
// Packing, any shape (WORD false): lane = (pixel p, slice z) of P = 64 / ZC pixels, so a wave loads
// consecutive bytes; __ballot packs them and lane p extracts its pixel's word; the store takes the
// word back from the lane that holds the column (__shfl) and writes consecutive bytes.
// Packing when Z is a multiple of 4 and at most 32 (WORD true: a pixel is Z / 4 aligned 32-bit words,
// and a tile row is one contiguous run of them): a lane loads its pixel's words and folds each into a
// nibble; for the store a wave lays a row's words out in LDS and writes them back 64 consecutive
// words at a time.
template <bool WORD>
__global__ void __launch_bounds__(ME_TPB) k_mask_morph(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                       const int32_t *__restrict__ radius, int64_t V, MeGeom g,
                                                       int erode) {
    __shared__ uint32_t s_x[(ME_TR + 2 * ME_KMAX) * ME_W];
    __shared__ uint32_t s_o[WORD ? ME_TPB * (ME_ZC_MAX / 4) : 1];   // WORD: 64 pixels x Z / 4 words per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = min(max(radius[blockIdx.y], 0), ME_KMAX);
    int bx = (int)blockIdx.x;
    const int zc = bx % g.nzc;
    bx /= g.nzc;
    const int ct = bx % g.nct, rt = bx / g.nct;
    const int r0 = rt * ME_TR, c0 = ct * ME_TC, z0 = zc * g.ZC;
    const int ZC = g.ZC, P = 64 / ZC;
    const int p = lane / ZC, z = lane - p * ZC;
    const bool zin = p < P && z0 + z < g.Z;
    const int nz = min(ZC, g.Z - z0);
    const uint32_t zmask = nz >= 32 ? 0xffffffffu : (1u << nz) - 1u;
    const int Q = g.Z >> 2;   // WORD: words per pixel (1..8)
    const uint8_t *xs = src + (int64_t)blockIdx.y * V;
    uint8_t *ys = dst + (int64_t)blockIdx.y * V;

    if (k == 0) {   // (the whole workgroup: k is per study)
        for (int o = wave; o < ME_TR; o += ME_TPB / 64) {
            const int gr = r0 + o;
            for (int j0 = 0; j0 < ME_TC; j0 += P) {
                const int gc = c0 + j0 + p;
                if (zin && j0 + p < ME_TC && gr < g.R && gc < g.C) {
                    const int64_t at = ((int64_t)gr * g.C + gc) * g.Z + z0 + z;
                    ys[at] = xs[at];
                }
            }
        }
        return;
    }

    // stage rows r0 - k .. r0 + ME_TR + k - 1, columns c0 - k .. c0 + ME_TC + k - 1 as words
    const int nrow = ME_TR + 2 * k, npix = ME_TC + 2 * k;
    const int sh = lane < P ? lane * ZC : 0;
    for (int i = wave; i < nrow; i += ME_TPB / 64) {
        const int gr = r0 - k + i;
        const bool rin = gr >= 0 && gr < g.R;
        if (WORD) {
            for (int j = lane; j < npix; j += 64) {
                const int gc = c0 - k + j;
                uint32_t w = 0u;
                if (rin && gc >= 0 && gc < g.C) {
                    const uint32_t *px = reinterpret_cast<const uint32_t *>(xs + ((int64_t)gr * g.C + gc) * g.Z);
#pragma unroll
                    for (int q = 0; q < ME_ZC_MAX / 4; ++q)
                        if (q < Q) w |= me_nib(px[q]) << (4 * q);
                    if (erode) w = ~w & zmask;
                }
                s_x[i * ME_W + j] = w;
            }
            continue;
        }
        for (int j0 = 0; j0 < npix; j0 += P) {   // (wave-uniform bounds: every lane reaches the ballot)
            const int gc = c0 - k + j0 + p;
            uint8_t v = 0;
            if (rin && zin && j0 + p < npix && gc >= 0 && gc < g.C)
                v = xs[((int64_t)gr * g.C + gc) * g.Z + z0 + z];
            const unsigned long long bal = __ballot(v != 0);
            const int gx = c0 - k + j0 + lane;   // the pixel whose word this lane extracts
            if (lane < P && j0 + lane < npix) {
                uint32_t w = (uint32_t)(bal >> sh) & zmask;
                if (erode) w = ~w & zmask;
                s_x[i * ME_W + j0 + lane] = (rin && gx >= 0 && gx < g.C) ? w : 0u;
            }
        }
    }
    __syncthreads();

    uint32_t acc[ME_SR];
#pragma unroll
    for (int o = 0; o < ME_SR; ++o) acc[o] = 0u;
    const int a = wave * ME_SR;
    switch (k) {
    case 1: me_dilate_strip<1>(s_x, a, lane, acc); break;
    case 2: me_dilate_strip<2>(s_x, a, lane, acc); break;
    case 3: me_dilate_strip<3>(s_x, a, lane, acc); break;
    case 4: me_dilate_strip<4>(s_x, a, lane, acc); break;
    default: me_dilate_strip<5>(s_x, a, lane, acc); break;
    }

    if (WORD) {
        // the row's words, pixel after pixel, in this wave's part of s_o; then 64 consecutive words
        // per store.  A lane past the last column writes LDS words that no store reads.
        uint32_t *so = s_o + wave * (64 * (ME_ZC_MAX / 4));
        const int nw = min(ME_TC, g.C - c0) * Q;
#pragma unroll
        for (int o = 0; o < ME_SR; ++o) {
            const uint32_t mine = erode ? ~acc[o] & zmask : acc[o];
            const int gr = r0 + a + o;
            if (gr >= g.R) break;   // (wave-uniform)
#pragma unroll
            for (int q = 0; q < ME_ZC_MAX / 4; ++q)
                if (q < Q) so[lane * Q + q] = me_unnib(mine >> (4 * q));
            me_wave_sync();
            uint32_t *row = reinterpret_cast<uint32_t *>(ys + ((int64_t)gr * g.C + c0) * g.Z);
            for (int d = lane; d < nw; d += 64) row[d] = so[d];
            me_wave_sync();
        }
        return;
    }
    // unpack: lane = (pixel p, slice z) again, the word comes from the lane that holds the column
#pragma unroll
    for (int o = 0; o < ME_SR; ++o) {
        const uint32_t mine = erode ? ~acc[o] & zmask : acc[o];
        const int gr = r0 + a + o;
        for (int j0 = 0; j0 < ME_TC; j0 += P) {
            const uint32_t w = __shfl(mine, min(j0 + p, 63), 64);
            const int gc = c0 + j0 + p;
            if (zin && j0 + p < ME_TC && gr < g.R && gc < g.C)
                ys[((int64_t)gr * g.C + gc) * g.Z + z0 + z] = (uint8_t)((w >> z) & 1u);
        }
    }
}

static MeGeom me_geometry(const vh_batch *b) {
    MeGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    g.ZC = (int)std::min<int64_t>(b->Z, ME_ZC_MAX);
    g.nct = (g.C + ME_TC - 1) / ME_TC;
    g.nzc = (g.Z + g.ZC - 1) / g.ZC;
    return g;
}

static int64_t me_blocks(const MeGeom &g) {
    return (int64_t)((g.R + ME_TR - 1) / ME_TR) * g.nct * g.nzc;
}

bool vh_mask_edit_takes(const vh_batch *b) {   // the grid: x in threads below 2^32, y
    return me_blocks(me_geometry(b)) < ((int64_t)1 << 24) && b->nb <= 65535;
}

void vh_mask_morph_launch(vh_batch *b, const uint8_t *src, uint8_t *dst, const int32_t *d_radius, int erode) {
    const MeGeom g = me_geometry(b);
    const dim3 grid((unsigned)me_blocks(g), (unsigned)b->nb, 1);
    ScopedKTimer tm(b, "mask_edit_b", 2.0 * (double)b->nb * (double)b->V);
    // (Z a multiple of 4 makes V one, and every study, row and pixel start on a 32-bit word)
    auto fn = (g.Z % 4 == 0 && g.nzc == 1) ? k_mask_morph<true> : k_mask_morph<false>;
    fn<<<grid, ME_TPB, 0, b->stream>>>(src, dst, d_radius, b->V, g, erode);
    VH_CHECK_LAUNCH();
}

__device__ __forceinline__ uint32_t me_paint(uint32_t s, uint32_t p, int how) {   // on 0 / 1 bytes
    return how == VH_PAINT_OR ? (s | p) : how == VH_PAINT_ANDNOT ? (s & ~p) : how == VH_PAINT_AND ? (s & p) : (s ^ p);
}

// mask = paint(mask != 0, strokes != 0) as 0 / 1 bytes, in place over the flat [nb * V] buffer (both
// buffers start on an allocation's boundary): n16 16-byte words, then the n - 16 n16 tail bytes
__global__ void k_mask_paint(uint8_t *__restrict__ mask, const uint8_t *__restrict__ strokes, int64_t n, int how,
                             unsigned long long *ks) {
    kst_begin(ks);
    const int64_t n16 = n >> 4;
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    uint4 *m4 = reinterpret_cast<uint4 *>(mask);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(strokes);
    for (int64_t i = t; i < n16; i += step) {
        const uint4 m = m4[i], s = s4[i];
        uint4 o;
        o.x = me_paint(me_nz01(m.x), me_nz01(s.x), how);
        o.y = me_paint(me_nz01(m.y), me_nz01(s.y), how);
        o.z = me_paint(me_nz01(m.z), me_nz01(s.z), how);
        o.w = me_paint(me_nz01(m.w), me_nz01(s.w), how);
        m4[i] = o;
    }
    const int64_t at = (n16 << 4) + t;
    if (at < n) mask[at] = (uint8_t)(me_paint(mask[at] != 0, strokes[at] != 0, how) & 1u);
    kst_end(ks);
}

void vh_mask_paint_launch(vh_batch *b, uint8_t *mask, const uint8_t *strokes, int how) {
    const int64_t n = b->nb * b->V;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((n >> 4) + ME_TPB - 1) / ME_TPB, 256 * 8));
    // stamped: the kernel follows the strokes' upload on the stream, and HIP events around a launch
    // that follows a copy took the copy's 30 ms into the span (measured on the bench batch)
    ScopedKTimer tm(b, "mask_edit_b", 2.0 * (double)n, true);
    k_mask_paint<<<(unsigned)blocks, ME_TPB, 0, b->stream>>>(mask, strokes, n, how, tm.stamp());
    VH_CHECK_LAUNCH();
}

// cnt[study] += voxels != 0 (cnt zeroed by the caller): grid (blocks, nb).  A study starts at any
// byte, so its bytes up to the first 16-byte boundary and after the last are read one by one.
__global__ void k_mask_count(const uint8_t *__restrict__ mask, int64_t V, unsigned long long *cnt) {
    const uint8_t *x = mask + (int64_t)blockIdx.y * V;
    const int64_t lead = (int64_t)((16u - (uint32_t)((uintptr_t)x & 15u)) & 15u);
    const int64_t head = lead < V ? lead : V;
    const int64_t n16 = (V - head) >> 4, tail0 = head + (n16 << 4);
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    const uint4 *x4 = reinterpret_cast<const uint4 *>(x + head);
    unsigned long long c = 0;
    for (int64_t i = t; i < n16; i += step) {
        const uint4 m = x4[i];
        c += __popc(me_nz01(m.x)) + __popc(me_nz01(m.y)) + __popc(me_nz01(m.z)) + __popc(me_nz01(m.w));
    }
    if (t < head) c += x[t] != 0;
    if (tail0 + t < V) c += x[tail0 + t] != 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt + blockIdx.y, c);
}

void vh_mask_count_launch(vh_batch *b, const uint8_t *mask, unsigned long long *d_cnt) {
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((b->V >> 4) + ME_TPB - 1) / ME_TPB, 64));
    for (int64_t y0 = 0; y0 < b->nb; y0 += 65535) {   // (grid y)
        const dim3 grid((unsigned)blocks, (unsigned)std::min<int64_t>(b->nb - y0, 65535), 1);
        k_mask_count<<<grid, ME_TPB, 0, b->stream>>>(mask + y0 * b->V, b->V, d_cnt + y0);
        VH_CHECK_LAUNCH();
    }
}
