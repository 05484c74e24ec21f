// defect_table.hip -- the defect table of a resident batch (vh_batch_defect_table): one row per
// component of the last vh_batch_components, largest first, with its integer moments, bounding box,
// exposed faces and fixed-point signal sums.  The spec is in include/vent_hip.h.  It reads the resident
// root and size maps (and the N4 volume) and writes buffers of its own.  Everything is an integer
// combined by integer add / min / max: no output depends on the order of the threads.
//
// A workgroup of the sweeps owns DT_CHUNK consecutive voxels of one study; thread t takes voxel
// chunk + k DT_TPB + t in round k, so a wave reads consecutive words.  On the batch's stream, no host wait:
//   k_dt_gather<false>  the qualifying roots (root[i] == i, size >= min_size): their number and voxels
//                   into stats, and their keys into the study's list of at most max_rows -- complete
//                   where n_qualifying <= max_rows, the common case, which the selection then skips
//   k_dt_hist / k_dt_scan   a study with more: a radix select of the max_rows-th greatest key, 11 bits a
//                   pass from the top of the 2 bv bits of (size, 2^bv - 1 - root), V < 2^bv: digit
//                   histograms in LDS, then one workgroup per study walks the bins from the top
//   k_dt_gather<true>   the keys at or above that cut-off into the list (keys differ: exactly max_rows)
//   k_dt_sort       a bitonic sort of the list in LDS, greatest key first: the row order; the rows are
//                   initialised here (root, size, the sentinels of the min columns; -1 in unused rows)
//   k_dt_accum      the sweep: a voxel finds its row by a binary search of its key in the sorted list
//                   (LDS), a thread sums the voxels of its current row in registers, a workgroup the
//                   rows of its chunk in DT_SLOTS LDS slots, and one global atomic per workgroup, row
//                   and column goes out; a row whose slot another row holds adds to global memory itself
//   k_dt_close      min_fx of a row without a counted voxel: the sentinel becomes 0
#include <algorithm>

#include "vh_internal.h"

#define DT_TPB 256
#define DT_VPT 16                          // voxels per thread
#define DT_CHUNK (DT_TPB * DT_VPT)         // voxels per workgroup
#define DT_UNROLL 8                        // rounds with their loads in flight together (divides DT_VPT)
#define DT_DBITS 11                        // bits of a radix-select digit
#define DT_BINS (1 << DT_DBITS)
#define DT_MAXP 6                          // passes: ceil(62 / 11)
#define DT_SLOTS 64                        // LDS rows of a workgroup of the sweep
#define DT_ACC 16                          // accumulated columns, 2..17
#define DT_SENT 0x7fffffffffffffffull      // a min column before its first voxel

static_assert(VH_DT_MAX_ROWS == 1024 && VH_DT_COLS == DT_ACC + 2, "the LDS lists and the column map");
static_assert(DT_VPT % DT_UNROLL == 0 && DT_BINS % DT_TPB == 0, "whole rounds");

typedef unsigned long long u64;

// the filter's key (components.hip): (size, -root), ordered as a 64-bit integer
__device__ __forceinline__ u64 dt_key(uint32_t size, int root) {
    return ((u64)size << 32) | (u64)(~(uint32_t)root);
}

// the same order in 2 bv bits (size <= V < 2^bv, root < V): what the radix select walks
__device__ __forceinline__ u64 dt_skey(uint32_t size, int root, int bv) {
    return ((u64)size << bv) | (u64)(((1u << bv) - 1u) - (uint32_t)root);
}

// whether the study needs the selection: more qualifying components than rows (stats[1] is complete
// once k_dt_gather<false> has ended)
__device__ __forceinline__ bool dt_selects(const u64 *stats, int64_t sb, int max_rows) {
    return stats[sb * 4 + 1] > (u64)max_rows;
}

// grid (chunks, nb).  FINAL = false: every qualifying root counts (stats[1] components, stats[3] voxels)
// and its key is listed; FINAL: the studies that select list the keys at or above their cut-off.  A
// workgroup stages its keys in LDS and takes its range of the list by one global atomic.  More than
// max_rows keys (not FINAL, a study that selects): the list's content is replaced later.
template <bool FINAL>
__global__ void __launch_bounds__(DT_TPB) k_dt_gather(const int *__restrict__ root, const uint32_t *__restrict__ size,
                                                      int64_t V, const uint32_t *__restrict__ min_size, u64 *stats,
                                                      const u64 *__restrict__ cutoff, uint32_t *cnt, u64 *keys,
                                                      int max_rows) {
    __shared__ u64 s_stage[VH_DT_MAX_ROWS];
    __shared__ u64 s_vox;
    __shared__ uint32_t s_n, s_base;
    const int64_t sb = blockIdx.y;
    if (FINAL && !dt_selects(stats, sb, max_rows)) return;   // (uniform over the workgroup)
    const int t = threadIdx.x;
    if (t == 0) {
        s_n = 0u;
        s_vox = 0ull;
    }
    __syncthreads();
    const uint32_t ms = min_size[sb];
    const u64 cut = FINAL ? cutoff[sb] : 0ull;
    const int *p = root + sb * V;
    const uint32_t *sz = size + sb * V;
    const int64_t base = (int64_t)blockIdx.x * DT_CHUNK + t;
    u64 vox = 0ull;
    for (int k0 = 0; k0 < DT_VPT; k0 += DT_UNROLL) {
        int rt[DT_UNROLL];
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {   // (a round past the volume reads its last voxel)
            const int64_t i = base + (int64_t)(k0 + q) * DT_TPB;
            rt[q] = p[i < V ? i : V - 1];
        }
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {
            const int64_t i = base + (int64_t)(k0 + q) * DT_TPB;
            if (i >= V || rt[q] != (int)i) continue;
            const uint32_t s = sz[i];
            if (s < ms) continue;
            const u64 key = dt_key(s, (int)i);
            if (key < cut) continue;
            vox += s;
            const uint32_t j = atomicAdd(&s_n, 1u);
            if (j < VH_DT_MAX_ROWS) s_stage[j] = key;
        }
    }
    if (!FINAL && vox) atomicAdd(&s_vox, vox);
    __syncthreads();
    const uint32_t nl = s_n;
    if (nl == 0u) return;
    if (t == 0) {
        s_base = atomicAdd(&cnt[sb], nl);
        if (!FINAL) {
            atomicAdd(&stats[sb * 4 + 1], (u64)nl);
            atomicAdd(&stats[sb * 4 + 3], s_vox);
        }
    }
    __syncthreads();
    const u64 b0 = s_base;
    const uint32_t ns = nl < VH_DT_MAX_ROWS ? nl : VH_DT_MAX_ROWS;
    for (uint32_t j = t; j < ns; j += DT_TPB)   // at most 4 rounds
        if (b0 + j < (u64)max_rows) keys[sb * VH_DT_MAX_ROWS + b0 + j] = s_stage[j];
}

// grid (chunks, nb), pass p of the studies that select: the digit (skey >> sh) & (2^w - 1) of every
// qualifying root whose bits above it equal the prefix the passes before chose.
__global__ void __launch_bounds__(DT_TPB) k_dt_hist(const int *__restrict__ root, const uint32_t *__restrict__ size,
                                                    int64_t V, const uint32_t *__restrict__ min_size,
                                                    const u64 *__restrict__ stats, const u64 *__restrict__ sel,
                                                    uint32_t *hist, int p, int sh, int w, int bv, int max_rows) {
    __shared__ uint32_t s_h[DT_BINS];
    const int64_t sb = blockIdx.y;
    if (!dt_selects(stats, sb, max_rows)) return;   // (uniform over the workgroup)
    const int t = threadIdx.x;
    for (int i = t; i < DT_BINS; i += DT_TPB) s_h[i] = 0u;
    __syncthreads();
    const uint32_t ms = min_size[sb];
    const u64 prefix = p ? sel[sb * 2] : 0ull;
    const int *rp = root + sb * V;
    const uint32_t *sz = size + sb * V;
    const int64_t base = (int64_t)blockIdx.x * DT_CHUNK + t;
    for (int k0 = 0; k0 < DT_VPT; k0 += DT_UNROLL) {
        int rt[DT_UNROLL];
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {
            const int64_t i = base + (int64_t)(k0 + q) * DT_TPB;
            rt[q] = rp[i < V ? i : V - 1];
        }
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {
            const int64_t i = base + (int64_t)(k0 + q) * DT_TPB;
            if (i >= V || rt[q] != (int)i) continue;
            const uint32_t s = sz[i];
            if (s < ms) continue;
            const u64 key = dt_skey(s, (int)i, bv);
            if ((key >> (sh + w)) != prefix) continue;   // (sh + w <= 2 bv <= 62; pass 0: nothing above)
            atomicAdd(&s_h[(uint32_t)(key >> sh) & ((1u << w) - 1u)], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < DT_BINS; i += DT_TPB)
        if (s_h[i]) atomicAdd(&hist[sb * DT_BINS + i], s_h[i]);
}

// grid (nb), pass p of the studies that select: sel = {prefix, k}, the key sought is the k-th greatest
// among those that begin with prefix.  Thread t owns the 8 digits from DT_BINS - 1 - 8 t downwards; the
// digit that holds the k-th extends the prefix, k loses the keys above it; the bins are zeroed for the
// next pass.  After the last pass the prefix is the key: the study's cut-off.
__global__ void __launch_bounds__(DT_TPB) k_dt_scan(uint32_t *hist, const u64 *__restrict__ stats, u64 *sel,
                                                    uint32_t *cnt, u64 *cutoff, int p, int w, int last, int bv,
                                                    int max_rows) {
    __shared__ uint32_t s_sum[DT_TPB];
    const int64_t sb = blockIdx.x;
    if (!dt_selects(stats, sb, max_rows)) return;   // (uniform over the workgroup)
    const int t = threadIdx.x;
    uint32_t *h = hist + sb * DT_BINS;
    const u64 prefix = p ? sel[sb * 2] : 0ull;
    const uint32_t k = p ? (uint32_t)sel[sb * 2 + 1] : (uint32_t)max_rows;
    constexpr int PER = DT_BINS / DT_TPB;
    uint32_t c[PER], sum = 0u;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        c[u] = h[DT_BINS - 1 - (PER * t + u)];
        sum += c[u];
    }
    s_sum[t] = sum;
    __syncthreads();
    for (int off = 1; off < DT_TPB; off <<= 1) {   // 8 steps: the inclusive scan of the threads' sums
        const uint32_t v = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    const uint32_t incl = s_sum[t], excl = incl - sum;
    if (excl < k && k <= incl) {   // one thread: the sums are those of at least k keys
        uint32_t above = excl, d = 0u;
        bool found = false;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (!found && above + c[u] >= k) {
                d = (uint32_t)(DT_BINS - 1 - (PER * t + u));
                found = true;
            }
            if (!found) above += c[u];
        }
        const u64 np = (prefix << w) | (u64)d;
        if (last) {
            const uint32_t mask = (1u << bv) - 1u;
            cutoff[sb] = dt_key((uint32_t)(np >> bv), (int)(mask - ((uint32_t)np & mask)));
        } else {
            sel[sb * 2] = np;
            sel[sb * 2 + 1] = (u64)(k - above);
        }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) h[DT_BINS - 1 - (PER * t + u)] = 0u;
    if (p == 0 && t == 0) cnt[sb] = 0u;   // the list is rebuilt by k_dt_gather<true>
}

// grid (nb): the study's list, greatest key first, and its rows before the sweep.  stats[0] = n_rows,
// stats[2] = the voxels in them.
__global__ void __launch_bounds__(DT_TPB) k_dt_sort(const uint32_t *__restrict__ cnt, u64 *keys, u64 *stats, u64 *rows,
                                                    int max_rows, int signal) {
    __shared__ u64 s_k[VH_DT_MAX_ROWS];
    __shared__ u64 s_vox;
    const int t = threadIdx.x;
    const int64_t sb = blockIdx.x;
    const int n = (int)min(cnt[sb], (uint32_t)max_rows);
    int np = 2;
    while (np < n) np <<= 1;   // bound: n <= 1024, at most 9 doublings
    for (int i = t; i < np; i += DT_TPB) s_k[i] = i < n ? keys[sb * VH_DT_MAX_ROWS + i] : 0ull;   // (a key is > 0)
    if (t == 0) s_vox = 0ull;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1)          // the bitonic network on np <= 1024 keys: 55 steps at the most
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < np; i += DT_TPB) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 a = s_k[i], b = s_k[l];
                    if ((i & k) == 0 ? a < b : a > b) {
                        s_k[i] = b;
                        s_k[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    u64 vox = 0ull;
    for (int j = t; j < n; j += DT_TPB) {
        keys[sb * VH_DT_MAX_ROWS + j] = s_k[j];
        vox += s_k[j] >> 32;
    }
    if (vox) atomicAdd(&s_vox, vox);
    u64 *rw = rows + sb * max_rows * VH_DT_COLS;
    for (int e = t; e < max_rows * VH_DT_COLS; e += DT_TPB) {   // at most 72 rounds
        const int j = e / VH_DT_COLS, col = e - j * VH_DT_COLS;
        u64 v = 0ull;
        if (j >= n) {
            v = col == 0 ? ~0ull : 0ull;   // -1
        } else if (col == 0) {
            v = (u64)(~(uint32_t)s_k[j]);
        } else if (col == 1) {
            v = s_k[j] >> 32;
        } else if (col == 5 || col == 7 || col == 9 || (col == 16 && signal)) {
            v = DT_SENT;
        }
        rw[e] = v;
    }
    __syncthreads();
    if (t == 0) {
        stats[sb * 4] = (u64)n;
        stats[sb * 4 + 2] = s_vox;
    }
}

// a thread's sums over the voxels of its current row, in the order of columns 2..17
struct DtAcc {
    u64 sr, sc, sz, sfx;
    uint32_t minr, maxr, minc, maxc, minz, maxz, fr, fc, fz, nsig, minfx, maxfx;
    __device__ __forceinline__ void reset() {
        sr = sc = sz = sfx = 0ull;
        minr = minc = minz = minfx = 0xffffffffu;
        maxr = maxc = maxz = fr = fc = fz = nsig = maxfx = 0u;
    }
};

// into a row's 16 accumulators, LDS or global (a voxel's coordinates and fx are below 2^31: the
// register sentinel 2^32 - 1 never goes out, since a flushed row has a voxel and nsig guards fx)
template <bool SIGNAL>
__device__ __forceinline__ void dt_push(u64 *dst, const DtAcc &a) {
    atomicAdd(dst + 0, a.sr);
    atomicAdd(dst + 1, a.sc);
    atomicAdd(dst + 2, a.sz);
    atomicMin(dst + 3, (u64)a.minr);
    atomicMax(dst + 4, (u64)a.maxr);
    atomicMin(dst + 5, (u64)a.minc);
    atomicMax(dst + 6, (u64)a.maxc);
    atomicMin(dst + 7, (u64)a.minz);
    atomicMax(dst + 8, (u64)a.maxz);
    atomicAdd(dst + 9, (u64)a.fr);
    atomicAdd(dst + 10, (u64)a.fc);
    atomicAdd(dst + 11, (u64)a.fz);
    if (SIGNAL && a.nsig) {
        atomicAdd(dst + 12, (u64)a.nsig);
        atomicAdd(dst + 13, a.sfx);
        atomicMin(dst + 14, (u64)a.minfx);
        atomicMax(dst + 15, (u64)a.maxfx);
    }
}

__device__ __forceinline__ bool dt_is_min(int col) { return col == 3 || col == 5 || col == 7 || col == 14; }
__device__ __forceinline__ bool dt_is_max(int col) { return col == 4 || col == 6 || col == 8 || col == 15; }

struct DtGeom {
    int R, C, Z;
    int64_t V;
};

// grid (chunks, nb).  nv = x / d is IEEE float32 division and nv * 2^24 one float32 multiply
// (-ffp-contract=off): the expressions of k_zn_count.
template <bool SIGNAL>
__global__ void __launch_bounds__(DT_TPB) k_dt_accum(const int *__restrict__ root, const uint32_t *__restrict__ size,
                                                     const float *__restrict__ x, const VolScalars *sc, DtGeom g,
                                                     int norm, const u64 *__restrict__ keys,
                                                     const u64 *__restrict__ stats, u64 *rows, int max_rows) {
    __shared__ u64 s_keys[VH_DT_MAX_ROWS];
    __shared__ u64 s_acc[DT_SLOTS * DT_ACC];
    __shared__ int s_tag[DT_SLOTS];
    const int64_t sb = blockIdx.y;
    const int n = (int)min(stats[sb * 4], (u64)max_rows);
    if (n == 0) return;   // (uniform over the workgroup)
    const int t = threadIdx.x;
    for (int i = t; i < n; i += DT_TPB) s_keys[i] = keys[sb * VH_DT_MAX_ROWS + i];   // at most 4 rounds
    for (int e = t; e < DT_SLOTS * DT_ACC; e += DT_TPB) s_acc[e] = dt_is_min(e % DT_ACC) ? ~0ull : 0ull;
    if (t < DT_SLOTS) s_tag[t] = -1;
    __syncthreads();
    const u64 least = s_keys[n - 1];
    const int *p = root + sb * g.V;
    const uint32_t *sz = size + sb * g.V;
    const float *xv = SIGNAL ? x + sb * g.V : nullptr;
    float d = 1.0f;
    if (SIGNAL) d = norm == VH_NORM_MEAN ? sc[sb].mean_anchor : sc[sb].p99;
    u64 *rw = rows + sb * max_rows * VH_DT_COLS;
    const int CZ = g.C * g.Z;   // (< V < 2^31)
    const int64_t base = (int64_t)blockIdx.x * DT_CHUNK + t;

    DtAcc a;
    a.reset();
    int cur = -1, last_root = -2;   // the row of last_root (-1: not in the table)
    auto flush = [&]() {
        if (cur < 0) return;
        const int slot = cur % DT_SLOTS;
        const int tag = atomicCAS(&s_tag[slot], -1, cur);
        if (tag == -1 || tag == cur) dt_push<SIGNAL>(s_acc + slot * DT_ACC, a);
        else dt_push<SIGNAL>(rw + (int64_t)cur * VH_DT_COLS + 2, a);
    };
    for (int k0 = 0; k0 < DT_VPT; k0 += DT_UNROLL) {
        int rt[DT_UNROLL];
        uint32_t sv[DT_UNROLL];
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {   // (a round past the volume reads its last voxel)
            const int64_t i = base + (int64_t)(k0 + q) * DT_TPB;
            const int64_t ic = i < g.V ? i : g.V - 1;
            rt[q] = p[ic];
            sv[q] = sz[ic];
        }
#pragma unroll
        for (int q = 0; q < DT_UNROLL; ++q) {
            const int64_t i64 = base + (int64_t)(k0 + q) * DT_TPB;
            const int r0 = rt[q];
            if (i64 >= g.V || r0 < 0) continue;
            if (r0 != last_root) {
                flush();
                a.reset();
                last_root = r0;
                cur = -1;
                const u64 key = dt_key(sv[q], r0);
                if (key >= least) {
                    int lo = 0, hi = n - 1;
                    for (int s = 0; s < 10; ++s) {   // n <= 1024: the interval is one key after 10 halvings
                        const int mid = (lo + hi) >> 1;
                        if (s_keys[mid] > key) lo = mid + 1;
                        else hi = mid;
                        if (lo >= hi) break;
                    }
                    if (s_keys[lo] == key) cur = lo;
                }
            }
            if (cur < 0) continue;
            const int i = (int)i64;
            const int z = i % g.Z, cq = i / g.Z, c = cq % g.C, r = cq / g.C;
            a.sr += (u64)r;
            a.sc += (u64)c;
            a.sz += (u64)z;
            a.minr = min(a.minr, (uint32_t)r);
            a.maxr = max(a.maxr, (uint32_t)r);
            a.minc = min(a.minc, (uint32_t)c);
            a.maxc = max(a.maxc, (uint32_t)c);
            a.minz = min(a.minz, (uint32_t)z);
            a.maxz = max(a.maxz, (uint32_t)z);
            // a neighbour is read only where it lies inside the volume
            a.fz += (z == 0 || p[i - 1] != r0) + (z == g.Z - 1 || p[i + 1] != r0);
            a.fc += (c == 0 || p[i - g.Z] != r0) + (c == g.C - 1 || p[i + g.Z] != r0);
            a.fr += (r == 0 || p[i - CZ] != r0) + (r == g.R - 1 || p[i + CZ] != r0);
            if (SIGNAL) {
                const float nv = xv[i] / d;
                if (nv >= 0.0f && nv < 64.0f) {
                    const uint32_t fx = (uint32_t)(long long)(nv * 16777216.0f);   // < 2^30
                    a.nsig += 1u;
                    a.sfx += (u64)fx;
                    a.minfx = min(a.minfx, fx);
                    a.maxfx = max(a.maxfx, fx);
                }
            }
        }
    }
    flush();
    __syncthreads();
    for (int e = t; e < DT_SLOTS * DT_ACC; e += DT_TPB) {   // 4 rounds
        const int slot = e / DT_ACC, col = e - slot * DT_ACC;
        const int row = s_tag[slot];
        if (row < 0) continue;
        const u64 v = s_acc[e];
        u64 *dst = rw + (int64_t)row * VH_DT_COLS + 2 + col;
        if (dt_is_min(col)) {
            if (v != ~0ull) atomicMin(dst, v);
        } else if (dt_is_max(col)) {
            if (v) atomicMax(dst, v);
        } else if (v) {
            atomicAdd(dst, v);
        }
    }
}

// grid (ceil(max_rows / DT_TPB), nb): a row with a component and n_sig = 0 still holds the sentinel
__global__ void __launch_bounds__(DT_TPB) k_dt_close(u64 *rows, int max_rows) {
    const int j = (int)(blockIdx.x * DT_TPB + threadIdx.x);
    if (j >= max_rows) return;
    u64 *row = rows + ((int64_t)blockIdx.y * max_rows + j) * VH_DT_COLS;
    if (row[14] == 0ull && row[16] == DT_SENT) row[16] = 0ull;
}

// grid y is the study, grid x the chunks (V < 2^31: far below 2^31 chunks)
bool vh_dt_takes(const vh_batch *b) { return b->nb <= 65535 && b->V < ((int64_t)1 << 31); }

void vh_dt_launch(vh_batch *b, int max_rows, int norm) {
    hipStream_t st = b->stream;
    const size_t nb = (size_t)b->nb;
    const bool signal = norm != VH_DT_NO_SIGNAL;
    const int *root = b->d_cc_root;
    const uint32_t *size = b->d_cc_size;
    HIP_TRY(hipMemsetAsync(b->d_dt_stats, 0, sizeof(u64) * nb * 4, st));
    HIP_TRY(hipMemsetAsync(b->d_dt_cut, 0, sizeof(u64) * nb, st));
    HIP_TRY(hipMemsetAsync(b->d_dt_cnt, 0, sizeof(uint32_t) * nb, st));
    HIP_TRY(hipMemsetAsync(b->d_dt_hist, 0, sizeof(uint32_t) * nb * DT_BINS, st));
    // the bytes the sweep has to move: the root and the size maps, and x with the signal columns
    ScopedKTimer tm(b, "dtab_b", (signal ? 12.0 : 8.0) * (double)b->nb * (double)b->V);
    const dim3 gv((unsigned)((b->V + DT_CHUNK - 1) / DT_CHUNK), (unsigned)b->nb, 1);
    const unsigned gs = (unsigned)b->nb;
    k_dt_gather<false><<<gv, DT_TPB, 0, st>>>(root, size, b->V, b->d_dt_min, b->d_dt_stats, b->d_dt_cut, b->d_dt_cnt,
                                              b->d_dt_keys, max_rows);
    VH_CHECK_LAUNCH();
    int bv = 1;
    while (((int64_t)1 << bv) <= b->V) ++bv;   // V < 2^bv, bv <= 31
    const int T = 2 * bv, passes = (T + DT_DBITS - 1) / DT_DBITS;   // <= DT_MAXP
    for (int p = 0; p < passes; ++p) {
        const int top = T - DT_DBITS * p, sh = std::max(top - DT_DBITS, 0), w = top - sh;
        k_dt_hist<<<gv, DT_TPB, 0, st>>>(root, size, b->V, b->d_dt_min, b->d_dt_stats, b->d_dt_sel, b->d_dt_hist, p, sh, w,
                                         bv, max_rows);
        VH_CHECK_LAUNCH();
        k_dt_scan<<<gs, DT_TPB, 0, st>>>(b->d_dt_hist, b->d_dt_stats, b->d_dt_sel, b->d_dt_cnt, b->d_dt_cut, p, w,
                                         p == passes - 1, bv, max_rows);
        VH_CHECK_LAUNCH();
    }
    k_dt_gather<true><<<gv, DT_TPB, 0, st>>>(root, size, b->V, b->d_dt_min, b->d_dt_stats, b->d_dt_cut, b->d_dt_cnt,
                                             b->d_dt_keys, max_rows);
    VH_CHECK_LAUNCH();
    k_dt_sort<<<gs, DT_TPB, 0, st>>>(b->d_dt_cnt, b->d_dt_keys, b->d_dt_stats, b->d_dt_rows, max_rows, signal ? 1 : 0);
    VH_CHECK_LAUNCH();
    DtGeom g;
    g.R = (int)b->R;
    g.C = (int)b->C;
    g.Z = (int)b->Z;
    g.V = b->V;
    if (signal) {
        k_dt_accum<true><<<gv, DT_TPB, 0, st>>>(root, size, b->n4_last(), b->d_sc, g, norm, b->d_dt_keys, b->d_dt_stats,
                                                b->d_dt_rows, max_rows);
        VH_CHECK_LAUNCH();
        const dim3 gc((unsigned)((max_rows + DT_TPB - 1) / DT_TPB), (unsigned)b->nb, 1);
        k_dt_close<<<gc, DT_TPB, 0, st>>>(b->d_dt_rows, max_rows);
        VH_CHECK_LAUNCH();
    } else {
        k_dt_accum<false><<<gv, DT_TPB, 0, st>>>(root, size, nullptr, b->d_sc, g, norm, b->d_dt_keys, b->d_dt_stats,
                                                 b->d_dt_rows, max_rows);
        VH_CHECK_LAUNCH();
    }
}
