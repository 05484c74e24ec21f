// dist.hip -- the ventilation distribution of a resident batch (vh_batch_distribution): per study the
// histogram of the normalised masked signal, and per slice the counts of mask, defect and the six
// linear-binning classes.  One read-only sweep over N4 (4 B), mask, defect map and LB classes (1 B
// each); only counts are written.  Every accumulation is an integer add, so the result does not
// depend on the order of the adds.
#include <algorithm>

#include "vh_internal.h"

#define DS_TPB 256
#ifndef DS_UNROLL
#define DS_UNROLL 8          // voxels per thread with their loads in flight together (4: 169 us for
#endif                       // the 256 x 128x128x24 batch, 8: 158 us, alternating in one session)
#define DS_COLS VH_DIST_COLS

// One voxel: its slice counters (cnt: the thread's registers or the workgroup's LDS row of the
// slice), the histogram bin or the outside counter.  nv = x / d is IEEE float32 division and
// nv * scale one float32 multiply (-ffp-contract=off), the expressions of k_cohort_search.
template <bool REG>
__device__ __forceinline__ void dist_voxel(float x, uint32_t m, uint32_t df, uint32_t l, float d, float hi,
                                           float scale, int n_bins, uint32_t *cnt, uint32_t *s_hist,
                                           uint32_t &out_lo, uint32_t &out_hi) {
    if (REG) {
        cnt[0] += m != 0u;
        cnt[1] += df != 0u;
#pragma unroll
        for (uint32_t c = 1; c <= 6; ++c) cnt[c + 1] += l == c;
    } else {   // (a class byte above 6 indexes nothing)
        if (m) atomicAdd(&cnt[0], 1u);
        if (df) atomicAdd(&cnt[1], 1u);
        if (l >= 1u && l <= 6u) atomicAdd(&cnt[l + 1u], 1u);
    }
    if (m) {
        const float nv = x / d;
        if (nv >= 0.0f && nv < hi) {
            int bi = (int)(nv * scale);
            bi = bi < 0 ? 0 : bi > n_bins - 1 ? n_bins - 1 : bi;
            atomicAdd(&s_hist[bi], 1u);
        } else if (nv < 0.0f) {
            ++out_lo;
        } else {   // nv >= hi, NaN: whatever a zero, infinite or NaN divisor gives included
            ++out_hi;
        }
    }
}

// grid (G, nb).  REG (Z <= DS_TPB): the first A = Z * (DS_TPB / Z) threads of a workgroup work, and
// thread t walks the voxels g A + t + k G A: A and G A are multiples of Z, so the thread stays on
// slice t % Z and its eight slice counters live in registers, while consecutive threads still read
// consecutive voxels.  Otherwise every thread strides by G DS_TPB and the slice counters are LDS
// atomics on s_sl [Z][8].  Either way the workgroup's counts go out once: LDS -> global integer
// atomics on the nonzero entries.
template <bool REG>
__global__ void __launch_bounds__(DS_TPB) k_dist(const float *__restrict__ n4, const uint8_t *__restrict__ mask,
                                                 const uint8_t *__restrict__ defect,
                                                 const uint8_t *__restrict__ lb, const VolScalars *sc,
                                                 int64_t V, int Z, int norm, int n_bins, float hi, float scale,
                                                 uint32_t *hist, unsigned long long *outside,
                                                 unsigned long long *slices) {
    extern __shared__ __align__(16) uint32_t s_dist[];
    uint32_t *s_hist = s_dist;                 // [n_bins]
    uint32_t *s_out = s_dist + n_bins;         // [2]
    uint32_t *s_sl = s_out + 2;                // [Z][DS_COLS]
    const int t = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int nsl = Z * DS_COLS;
    for (int i = t; i < n_bins + 2 + nsl; i += DS_TPB) s_dist[i] = 0u;
    __syncthreads();
    const float d = norm == VH_NORM_MEAN ? sc[b].mean_anchor : sc[b].p99;
    const int A = REG ? Z * (DS_TPB / Z) : DS_TPB;
    const int64_t stride = (int64_t)gridDim.x * A;
    const float *x = n4 + b * V;
    const uint8_t *mk = mask + b * V, *df = defect + b * V, *cl = lb + b * V;
    uint32_t cnt[DS_COLS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t out_lo = 0u, out_hi = 0u;
    if (t < A) {
        int64_t i = (int64_t)blockIdx.x * A + t;
        for (; i + (DS_UNROLL - 1) * stride < V; i += DS_UNROLL * stride) {
            float xv[DS_UNROLL];
            uint32_t mv[DS_UNROLL], dv[DS_UNROLL], lv[DS_UNROLL];
#pragma unroll
            for (int q = 0; q < DS_UNROLL; ++q) {
                const int64_t j = i + q * stride;
                xv[q] = x[j]; mv[q] = mk[j]; dv[q] = df[j]; lv[q] = cl[j];
            }
#pragma unroll
            for (int q = 0; q < DS_UNROLL; ++q) {
                // (j < V < 2^31, check_dims: a 32-bit remainder)
                uint32_t *c = REG ? cnt : s_sl + (uint32_t)((uint32_t)(i + q * stride) % (uint32_t)Z) * DS_COLS;
                dist_voxel<REG>(xv[q], mv[q], dv[q], lv[q], d, hi, scale, n_bins, c, s_hist, out_lo, out_hi);
            }
        }
        for (; i < V; i += stride) {
            uint32_t *c = REG ? cnt : s_sl + (uint32_t)((uint32_t)i % (uint32_t)Z) * DS_COLS;
            dist_voxel<REG>(x[i], mk[i], df[i], cl[i], d, hi, scale, n_bins, c, s_hist, out_lo, out_hi);
        }
        if (REG) {
            uint32_t *row = s_sl + (t % Z) * DS_COLS;
#pragma unroll
            for (int c = 0; c < DS_COLS; ++c)
                if (cnt[c]) atomicAdd(&row[c], cnt[c]);
        }
        if (out_lo) atomicAdd(&s_out[0], out_lo);
        if (out_hi) atomicAdd(&s_out[1], out_hi);
    }
    __syncthreads();
    for (int i = t; i < n_bins; i += DS_TPB)
        if (s_hist[i]) atomicAdd(&hist[b * n_bins + i], s_hist[i]);
    if (t < 2 && s_out[t]) atomicAdd(&outside[b * 2 + t], (unsigned long long)s_out[t]);
    for (int i = t; i < nsl; i += DS_TPB)
        if (s_sl[i]) atomicAdd(&slices[b * nsl + i], (unsigned long long)s_sl[i]);
}

bool vh_dist_takes(const vh_batch *b) { return b->Z <= VH_DIST_MAX_Z; }

void vh_dist_launch(vh_batch *b, int norm, int n_bins, float hi, float scale) {
    hipStream_t st = b->stream;
    const int Z = (int)b->Z;
    const bool reg = Z <= DS_TPB;
    const int64_t A = reg ? (int64_t)Z * (DS_TPB / Z) : DS_TPB;
    // several workgroups per study (a batch of one study still fills the device), about 2048 in all:
    // every workgroup flushes up to n_bins + 8 Z counts, so few voxels per workgroup would make the
    // flush the larger part
    const int64_t want = (b->V + A * DS_UNROLL - 1) / (A * DS_UNROLL), cap = (2048 + b->nb - 1) / b->nb;
    const int64_t G = std::max<int64_t>(1, std::min(want, cap));
    const size_t lds = sizeof(uint32_t) * ((size_t)n_bins + 2 + (size_t)Z * DS_COLS);
    HIP_TRY(hipMemsetAsync(b->d_dist_hist, 0, sizeof(uint32_t) * (size_t)b->nb * n_bins, st));
    HIP_TRY(hipMemsetAsync(b->d_dist_out, 0, sizeof(unsigned long long) * (size_t)b->nb * 2, st));
    HIP_TRY(hipMemsetAsync(b->d_dist_sl, 0, sizeof(unsigned long long) * (size_t)b->nb * Z * DS_COLS, st));
    ScopedKTimer tm(b, "dist_b", 7.0 * (double)b->nb * (double)b->V);
    const dim3 grid((unsigned)G, (unsigned)b->nb, 1);
    if (reg)
        k_dist<true><<<grid, DS_TPB, lds, st>>>(b->n4_last(), b->d_mask, b->d_defect, b->d_lb, b->d_sc, b->V, Z,
                                                norm, n_bins, hi, scale, b->d_dist_hist, b->d_dist_out,
                                                b->d_dist_sl);
    else
        k_dist<false><<<grid, DS_TPB, lds, st>>>(b->n4_last(), b->d_mask, b->d_defect, b->d_lb, b->d_sc, b->V, Z,
                                                 norm, n_bins, hi, scale, b->d_dist_hist, b->d_dist_out,
                                                 b->d_dist_sl);
    VH_CHECK_LAUNCH();
}
