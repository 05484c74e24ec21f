// denoise.hip -- the in-plane non-local-means denoise of a resident batch (vh_batch_denoise) and the
// per-study noise estimate behind it (vh_batch_noise_sigma); the spec is in include/vent_hip.h.
// Every operation of the filter is a correctly-rounded float32 add, subtract, multiply, divide or
// square root in a fixed order (-ffp-contract=off: no fused multiply-add), so tests/denoise_ref.py
// reproduces the output to the last bit.
#include <algorithm>

#include "vh_internal.h"

#define DN_TPB 256
#define DN_TR 16             // output rows per workgroup: one thread walks them down its column
#define DN_ZC_MAX 32         // slices per workgroup (all of them when Z <= 32)

struct DnGeom {
    int R, C, Z;
    int S;
    int ZC, TC;              // slices / columns per tile: TC * ZC <= DN_TPB threads work
    int nct, nzc;            // column tiles, slice chunks (blockIdx.x = (row tile * nct + column tile) * nzc + chunk)
    int W;                   // floats per staged row: (TC + 2 (S + P)) * ZC
};

// One launch over the batch: grid (row tiles x column tiles x slice chunks, nb).
//
// LDS holds the workgroup's tile of the edge-padded study with a halo of H = S + P,
// s_x[row][column][slice], the slice fastest as in HBM: thread t = column * ZC + slice of the tile
// reads s_x[constant + t], so a wave's 64 lanes read 64 consecutive words whatever the search and
// patch offsets are (no bank conflict), and the staging loads walk whole contiguous row segments.
//
// For one search offset d the squared difference e(a) = (X(a) - X(a + d))^2 of a pixel pair is the
// same float in every patch that holds a.  A thread walks its column down the tile's rows and keeps
// the (2P+1) x (2P+1) window of e in registers: each new row costs 2P+1 pairs, not (2P+1)^2, and the
// voxel's d2 is the window summed in raster order (ur outer), the order the spec fixes.  d2 starts
// at e[0][0]: +0 + e is e for every e, because a square is never -0.
template <int P, bool RICIAN>
__global__ void __launch_bounds__(DN_TPB) k_denoise_b(const float *__restrict__ x, float *__restrict__ out,
                                                      const float2 *__restrict__ prm, int64_t V, DnGeom g) {
    extern __shared__ __align__(16) float s_x[];
    constexpr int PW = 2 * P + 1;
    const int t = threadIdx.x;
    const int H = g.S + P, W = g.W, ZC = g.ZC;
    int bx = (int)blockIdx.x;
    const int zc = bx % g.nzc;
    bx /= g.nzc;
    const int ct = bx % g.nct, rt = bx / g.nct;
    const int r0 = rt * DN_TR, c0 = ct * g.TC, z0 = zc * ZC;
    const int tc = t / ZC, tz = t - tc * ZC;
    const float *xs = x + (int64_t)blockIdx.y * V;

    // stage rows r0 - H .. r0 + DN_TR + H - 1, columns c0 - H .. c0 + TC + H - 1, slices z0 .. z0 + ZC - 1,
    // every index clamped into the study (np.pad(mode='edge'); a slice past Z - 1 repeats the last
    // one and is never written): element e of a row is (column e / ZC, slice e % ZC), advanced by
    // DN_TPB per step without a division
    {
        const int qs = DN_TPB / ZC, rs = DN_TPB - qs * ZC;
        const int64_t CZ = (int64_t)g.C * g.Z;
        for (int i = 0; i < DN_TR + 2 * H; ++i) {
            const int gr = min(max(r0 - H + i, 0), g.R - 1);
            const float *row = xs + gr * CZ;
            int jc = tc, jz = tz;
            for (int e = t; e < W; e += DN_TPB) {
                const int gc = min(max(c0 - H + jc, 0), g.C - 1), gz = min(z0 + jz, g.Z - 1);
                s_x[i * W + e] = row[(int64_t)gc * g.Z + gz];
                jc += qs;
                jz += rs;
                if (jz >= ZC) { jz -= ZC; ++jc; }
            }
        }
    }
    __syncthreads();
    if (tc >= g.TC || c0 + tc >= g.C || z0 + tz >= g.Z) return;   // (no barrier below)

    const float2 pr = prm[blockIdx.y];
    const float inv_h2 = pr.x, bias = pr.y;
    // tile pixel (row i, column tc + j) for this thread: base[i * W + j * ZC], i in [-H, DN_TR + H),
    // j in [-H, H]: inside the staged tile by construction
    const float *base = s_x + H * W + H * ZC + t;
    float num[DN_TR], den[DN_TR];
#pragma unroll
    for (int o = 0; o < DN_TR; ++o) num[o] = den[o] = 0.0f;

    for (int dr = -g.S; dr <= g.S; ++dr)
        for (int dc = -g.S; dc <= g.S; ++dc) {
            const float *pa = base, *pb = base + dr * W + dc * ZC;
            float e[PW][PW] = {};
#pragma unroll
            for (int i = -P; i < DN_TR + P; ++i) {
#pragma unroll
                for (int k = 0; k + 1 < PW; ++k)
#pragma unroll
                    for (int j = 0; j < PW; ++j) e[k][j] = e[k + 1][j];
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    const float d = pa[i * W + (j - P) * ZC] - pb[i * W + (j - P) * ZC];
                    e[PW - 1][j] = d * d;
                }
                if (i >= P) {   // the window is rows o - P .. o + P of output row o
                    const int o = i - P;
                    float d2 = e[0][0];
#pragma unroll
                    for (int k = 0; k < PW; ++k)
#pragma unroll
                        for (int j = 0; j < PW; ++j)
                            if (k + j > 0) d2 = d2 + e[k][j];
                    const float u = d2 * inv_h2;
                    const float v = 1.0f - u;
                    const float w = u < 1.0f ? v * v : 0.0f;   // (NaN: 0)
                    float y = pb[o * W];
                    if (RICIAN) y = y * y;
                    num[o] = num[o] + w * y;   // also when w == 0: an infinite y gives NaN, as in numpy
                    den[o] = den[o] + w;
                }
            }
        }

    float *dst = out + (int64_t)blockIdx.y * V + ((int64_t)r0 * g.C + (c0 + tc)) * g.Z + (z0 + tz);
    const int64_t CZ = (int64_t)g.C * g.Z;
#pragma unroll
    for (int o = 0; o < DN_TR; ++o) {
        float r = num[o] / den[o];
        if (RICIAN) {
            const float v = r - bias;
            r = v > 0.0f ? sqrtf(v) : 0.0f;
        }
        if (r0 + o < g.R) dst[o * CZ] = r;
    }
}

static DnGeom dn_geometry(const vh_batch *b, int S, int P) {
    DnGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    g.S = S;
    g.ZC = (int)std::min<int64_t>(b->Z, DN_ZC_MAX);
    g.TC = (int)std::min<int64_t>(DN_TPB / g.ZC, b->C);
    g.nct = (g.C + g.TC - 1) / g.TC;
    g.nzc = (g.Z + g.ZC - 1) / g.ZC;
    g.W = (g.TC + 2 * (S + P)) * g.ZC;
    return g;
}

static int64_t dn_blocks(const DnGeom &g) {
    return (int64_t)((g.R + DN_TR - 1) / DN_TR) * g.nct * g.nzc;
}

bool vh_denoise_takes(const vh_batch *b) {   // the grid: x in threads below 2^32 (the radii do not change it), y
    return dn_blocks(dn_geometry(b, 1, 0)) < ((int64_t)1 << 24) && b->nb <= 65535;
}

void vh_denoise_launch(vh_batch *b, const float *src, float *dst, const float *d_prm, int S, int P, int rician) {
    const DnGeom g = dn_geometry(b, S, P);
    // at most (16 + 14) rows of (256 + 14 * 32) floats: 84 480 bytes of the CU's 160 KiB
    const size_t lds = sizeof(float) * (size_t)(DN_TR + 2 * (S + P)) * g.W;
    const dim3 grid((unsigned)dn_blocks(g), (unsigned)b->nb, 1);
    auto fn = rician ? (P == 0 ? k_denoise_b<0, true> : P == 1 ? k_denoise_b<1, true> : k_denoise_b<2, true>)
                     : (P == 0 ? k_denoise_b<0, false> : P == 1 ? k_denoise_b<1, false> : k_denoise_b<2, false>);
    vh_set_max_lds((const void *)fn, 96 * 1024);
    ScopedKTimer tm(b, "denoise_b", 8.0 * (double)b->nb * (double)b->V);
    fn<<<grid, DN_TPB, lds, b->stream>>>(src, dst, reinterpret_cast<const float2 *>(d_prm), b->V, g);
    VH_CHECK_LAUNCH();
}

// sigma = float32(sqrt(S2 / (2 N))) from the SNR sweep's double partials (part[..][2] the noise
// voxels' sum of squares, [3] their count), summed as k_snr_finish sums them: one wave per study,
// lane l takes parts l, l + 64, ... in order, then a fixed shuffle tree.  NaN where the SNR is
// undefined (no masked column > 0, or no noise voxel).
__global__ void k_noise_sigma(const double *part, int64_t nparts, int64_t nb, const VolScalars *sc,
                              float *sigma) {
    const int64_t b = blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= nb) return;
    double s2 = 0.0, n = 0.0;
    for (int64_t p = lane; p < nparts; p += 64) {
        s2 += part[(b * nparts + p) * 4 + 2];
        n += part[(b * nparts + p) * 4 + 3];
    }
    for (int off = 32; off > 0; off >>= 1) {
        s2 += __shfl_xor(s2, off, 64);
        n += __shfl_xor(n, off, 64);
    }
    if (lane != 0) return;
    sigma[b] = (!sc[b].snr_ok || n <= 0.0) ? __uint_as_float(0x7fc00000u) : (float)sqrt(s2 / (2.0 * n));
}

void vh_noise_sigma_launch(vh_batch *b, float *d_sigma) {
    k_noise_sigma<<<(unsigned)((b->nb + 3) / 4), 256, 0, b->stream>>>(b->d_snrpart, b->slab_blocks, b->nb,
                                                                     b->d_sc, d_sigma);
    VH_CHECK_LAUNCH();
}
