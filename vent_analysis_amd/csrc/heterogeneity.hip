// heterogeneity.hip -- the local ventilation heterogeneity of a resident batch (vh_batch_heterogeneity):
// per voxel the coefficient of variation of the signal over the masked pixels of a (2k+1) x (2k+1)
// in-plane window, and per study its histogram, three counts and a fixed-point sum; the spec is in
// include/vent_hip.h.  Every operation of the map is a correctly-rounded float32 add, subtract,
// multiply, divide or square root in a fixed order (-ffp-contract=off: no fused multiply-add), so
// tests/heterogeneity_ref.py reproduces it to the last bit; every accumulation of the summary is an
// integer add, so it does not depend on the order of the adds.
#include <algorithm>

#include "vh_internal.h"

#define HT_TPB 256
#define HT_TR 16             // output rows per workgroup: one thread walks them down its column
#define HT_ZC_MAX 32         // slices per workgroup (all of them when Z <= 32)
#define HT_STAGE 4           // staged elements per thread with their loads in flight together
#define HT_HEAD 8            // words in front of the histogram: the 64-bit sum, three counts, one unused

struct HtGeom {
    int R, C, Z;
    int ZC, TC;              // slices / columns per tile: TC * ZC <= HT_TPB threads work
    int nct, nzc;            // column tiles, slice chunks (blockIdx.x = (row tile * nct + column tile) * nzc + chunk)
    int W;                   // elements per staged row: (TC + 2 K) * ZC
};

// One launch over the batch: grid (row tiles x column tiles x slice chunks, nb).
//
// LDS holds the workgroup's tile with a halo of K, s_x[row][column][slice] (the raw words of x) and
// s_m[row][column][slice] (the effective mask M as 0 / 1 bytes), the slice fastest as in HBM: thread
// t = column * ZC + slice of the tile reads s_x[constant + t], so a wave's 64 lanes read 64
// consecutive words whatever the window offset is (no bank conflict), and the staging loads walk
// whole contiguous row segments.  Outside the slice M is 0 (and x +0, never read into a sum): there is
// no clamping and no padding value.
//
// A thread walks its column down the tile's rows.  It keeps the window's mask in registers, one word
// per window row (bit j = column offset j - K), so each new output row costs 2K+1 byte reads, and
// n is a population count.  A voxel with M clear writes +0 and skips the window; the others walk it
// twice from LDS, once for s and once for q, each a conditional add in raster order.
//
// The summary is fused: the thread's voxels go to the workgroup's LDS histogram and to its own three
// counts and fixed-point sum, which end in LDS by integer atomics; the workgroup then adds its
// nonzero words to the study's rows (32-bit adds for the bins, 64-bit adds for stats).
template <int K>
__global__ void __launch_bounds__(HT_TPB) k_het_b(const float *__restrict__ x, const uint8_t *__restrict__ mask,
                                                  const uint8_t *__restrict__ defect, float *__restrict__ out,
                                                  int64_t V, HtGeom g, int min_count, int n_bins, float hi,
                                                  float scale, uint32_t *hist, unsigned long long *stats) {
    extern __shared__ __align__(16) uint32_t s_het[];
    constexpr int KW = 2 * K + 1;
    unsigned long long *s_sum = reinterpret_cast<unsigned long long *>(s_het);   // [1]
    uint32_t *s_cnt = s_het + 2;                                                   // [3]: n_in, n_over, n_none
    uint32_t *s_hist = s_het + HT_HEAD;                                            // [n_bins]
    const int t = threadIdx.x;
    const int W = g.W, ZC = g.ZC;
    float *s_x = reinterpret_cast<float *>(s_hist + n_bins);                       // [HT_TR + 2 K][W]
    uint8_t *s_m = reinterpret_cast<uint8_t *>(s_x + (HT_TR + 2 * K) * W);         // [HT_TR + 2 K][W]
    int bx = (int)blockIdx.x;
    const int zc = bx % g.nzc;
    bx /= g.nzc;
    const int ct = bx % g.nct, rt = bx / g.nct;
    const int r0 = rt * HT_TR, c0 = ct * g.TC, z0 = zc * ZC;
    const int tc = t / ZC, tz = t - tc * ZC;
    const int64_t sb = blockIdx.y;
    const float *xs = x + sb * V;
    const uint8_t *ms = mask + sb * V;
    const uint8_t *ds = defect ? defect + sb * V : nullptr;

    for (int i = t; i < HT_HEAD + n_bins; i += HT_TPB) s_het[i] = 0u;
    // stage rows r0 - K .. r0 + HT_TR + K - 1, columns c0 - K .. c0 + TC + K - 1, slices z0 .. z0 + ZC - 1:
    // the tile is one run of (HT_TR + 2 K) W elements, element e = (row e / W, column (e % W) / ZC,
    // slice e % ZC), walked by all threads with HT_STAGE loads of each volume in flight per thread (a
    // row is shorter than two workgroups' width at Z = 24, so a loop per row would leave most of its
    // second step idle); whatever lies outside the study is M = 0
    {
        const uint32_t total = (uint32_t)((HT_TR + 2 * K) * W);
        const int64_t CZ = (int64_t)g.C * g.Z;
        for (uint32_t e0 = (uint32_t)t; e0 < total; e0 += HT_STAGE * HT_TPB) {
            float xv[HT_STAGE];
            uint32_t mv[HT_STAGE], dv[HT_STAGE];
#pragma unroll
            for (int u = 0; u < HT_STAGE; ++u) {
                const uint32_t e = e0 + (uint32_t)u * HT_TPB;
                const uint32_t i = e / (uint32_t)W, rem = e - i * (uint32_t)W;
                const uint32_t jc = rem / (uint32_t)ZC, jz = rem - jc * (uint32_t)ZC;
                const int gr = r0 - K + (int)i, gc = c0 - K + (int)jc, gz = z0 + (int)jz;
                xv[u] = 0.0f;
                mv[u] = dv[u] = 0u;
                if (e < total && gr >= 0 && gr < g.R && gc >= 0 && gc < g.C && gz < g.Z) {
                    const int64_t a = (int64_t)gr * CZ + (int64_t)gc * g.Z + gz;
                    xv[u] = xs[a];
                    mv[u] = ms[a];
                    if (ds) dv[u] = ds[a];
                }
            }
#pragma unroll
            for (int u = 0; u < HT_STAGE; ++u) {
                const uint32_t e = e0 + (uint32_t)u * HT_TPB;
                if (e < total) {
                    s_x[e] = xv[u];
                    s_m[e] = (uint8_t)(mv[u] != 0u && dv[u] == 0u);
                }
            }
        }
    }
    __syncthreads();

    uint32_t n_in = 0u, n_over = 0u, n_none = 0u;
    unsigned long long sum_fx = 0ull;
    if (tc < g.TC && c0 + tc < g.C && z0 + tz < g.Z) {
        // the window's top left pixel of output row o for this thread: s_x[o * W + t], its pixel
        // (window row i, window column j) at + i * W + j * ZC: inside the staged tile by construction
        const float *bx0 = s_x + t;
        const uint8_t *bm0 = s_m + t;
        uint32_t bits[KW];
        bits[0] = 0u;
#pragma unroll
        for (int i = 0; i + 1 < KW; ++i) {   // staged rows 0 .. 2K - 1; the walk shifts them up by one
            uint32_t w = 0u;
#pragma unroll
            for (int j = 0; j < KW; ++j) w |= (uint32_t)bm0[i * W + j * ZC] << j;
            bits[i + 1] = w;
        }
        const int64_t CZ = (int64_t)g.C * g.Z;
        float *dst = out + sb * V + ((int64_t)r0 * g.C + (c0 + tc)) * g.Z + (z0 + tz);
        const int rows = min(HT_TR, g.R - r0);
#pragma unroll 1
        for (int o = 0; o < rows; ++o) {
            const float *px = bx0 + o * W;
            {
                uint32_t w = 0u;
#pragma unroll
                for (int j = 0; j < KW; ++j) w |= (uint32_t)bm0[(o + KW - 1) * W + j * ZC] << j;
#pragma unroll
                for (int i = 0; i + 1 < KW; ++i) bits[i] = bits[i + 1];
                bits[KW - 1] = w;
            }
            float r = 0.0f;
            if ((bits[K] >> K) & 1u) {
                int n = 0;
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < KW; ++i) {
                    n += __popc(bits[i]);
#pragma unroll
                    for (int j = 0; j < KW; ++j) {
                        const float xv = px[i * W + j * ZC];
                        s = ((bits[i] >> j) & 1u) ? s + xv : s;
                    }
                }
                const float m = s / (float)n;
                float q = 0.0f;
#pragma unroll
                for (int i = 0; i < KW; ++i)
#pragma unroll
                    for (int j = 0; j < KW; ++j) {
                        const float d = px[i * W + j * ZC] - m;
                        const float dd = d * d;
                        q = ((bits[i] >> j) & 1u) ? q + dd : q;
                    }
                if (n >= min_count && m > 0.0f) {
                    r = sqrtf(q / (float)(n - 1)) / m;
                    if (r < hi) {
                        int bi = (int)(r * scale);
                        bi = bi < 0 ? 0 : bi > n_bins - 1 ? n_bins - 1 : bi;
                        atomicAdd(&s_hist[bi], 1u);
                        ++n_in;
                        sum_fx += (unsigned long long)(long long)(r * 16777216.0f);
                    } else {   // r >= hi, NaN
                        ++n_over;
                    }
                } else {
                    r = -1.0f;
                    ++n_none;
                }
            }
            dst[o * CZ] = r;
        }
    }
    if (n_in) atomicAdd(&s_cnt[0], n_in);
    if (n_over) atomicAdd(&s_cnt[1], n_over);
    if (n_none) atomicAdd(&s_cnt[2], n_none);
    if (sum_fx) atomicAdd(s_sum, sum_fx);
    __syncthreads();
    for (int i = t; i < n_bins; i += HT_TPB)
        if (s_hist[i]) atomicAdd(&hist[sb * n_bins + i], s_hist[i]);
    if (t < 3 && s_cnt[t]) atomicAdd(&stats[sb * 4 + t], (unsigned long long)s_cnt[t]);
    if (t == 3 && *s_sum) atomicAdd(&stats[sb * 4 + 3], *s_sum);
}

static HtGeom ht_geometry(const vh_batch *b, int K) {
    HtGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    g.ZC = (int)std::min<int64_t>(b->Z, HT_ZC_MAX);
    g.TC = (int)std::min<int64_t>(HT_TPB / g.ZC, b->C);
    g.nct = (g.C + g.TC - 1) / g.TC;
    g.nzc = (g.Z + g.ZC - 1) / g.ZC;
    g.W = (g.TC + 2 * K) * g.ZC;
    return g;
}

static int64_t ht_blocks(const HtGeom &g) {
    return (int64_t)((g.R + HT_TR - 1) / HT_TR) * g.nct * g.nzc;
}

bool vh_het_takes(const vh_batch *b) {   // the grid: x in threads below 2^32 (the radius does not change it), y
    return ht_blocks(ht_geometry(b, 1)) < ((int64_t)1 << 24) && b->nb <= 65535;
}

void vh_het_launch(vh_batch *b, const float *src, const uint8_t *defect, float *map, uint32_t *d_hist,
                   unsigned long long *d_stats, int K, int min_count, int n_bins, float hi, float scale) {
    hipStream_t st = b->stream;
    const HtGeom g = ht_geometry(b, K);
    // at most 32 + 4096 bytes in front of (16 + 10) rows of (256 + 10 * 32) elements of 5 bytes:
    // 79 008 bytes of the CU's 160 KiB
    const size_t lds = sizeof(uint32_t) * (size_t)(HT_HEAD + n_bins) + 5 * (size_t)(HT_TR + 2 * K) * g.W;
    HIP_TRY(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * (size_t)b->nb * n_bins, st));
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * (size_t)b->nb * 4, st));
    const dim3 grid((unsigned)ht_blocks(g), (unsigned)b->nb, 1);
    auto fn = K == 1 ? k_het_b<1> : K == 2 ? k_het_b<2> : K == 3 ? k_het_b<3> : K == 4 ? k_het_b<4> : k_het_b<5>;
    vh_set_max_lds((const void *)fn, 96 * 1024);
    ScopedKTimer tm(b, "het_b", (defect ? 10.0 : 9.0) * (double)b->nb * (double)b->V);
    fn<<<grid, HT_TPB, lds, st>>>(src, b->d_mask, defect, map, b->V, g, min_count, n_bins, hi, scale, d_hist,
                                  d_stats);
    VH_CHECK_LAUNCH();
}
