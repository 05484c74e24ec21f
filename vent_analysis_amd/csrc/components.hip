// components.hip -- the connected components of one resident byte volume per study
// (vh_batch_components / vh_batch_filter_components): per voxel of S = (a != 0) the component's root,
// the smallest linear index of the component, and its size; per study the number of set voxels and of
// components, the largest component, and the components and voxels of every size class; and the filter
// that clears the components below a size or beyond the k largest.  The spec is in include/vent_hip.h.
// Everything is an integer combined by integer atomics (min, max, add): the result does not depend on
// the order of the threads.
//
// A union-find over a parent array with the invariant parent[i] <= i (parent[i] == i: a root), so the
// root of a set is its smallest index -- the canonical label -- and every walk towards a root strictly
// decreases: no input can make one spin.
//   k_cc_local    a workgroup takes a tile of 16 x 16 x (up to 24) voxels, the whole of Z where
//                 Z <= 24 so that its rows are contiguous bytes, labels it in LDS (runs along Z, or
//                 along C for the per-slice connectivities, by a walk; then a union per in-tile link to
//                 a voxel before it in index order that the run before it does not imply already, an
//                 LDS atomicMin on the larger root)
//                 and writes the tile's roots as linear indices of the study, with the voxel count
//                 of every tile-local component at its tile-local root.
//   k_cc_merge    the voxels next to a tile face unite across it, diagonal links over tile edges and
//                 corners included, in the global parent array -- the int32 root map itself.
//   k_cc_flatten  root[i] = find(i); a tile-local root that is not its component's root adds its count
//                 to the root's: one global atomic per tile-local component, not per voxel.
//   k_cc_summary  size[i] = size[root[i]], and where root[i] == i the component is counted: classes
//                 through LDS, the largest by a 64-bit atomicMax of (size << 32 | ~root).
//   k_cc_pick / k_cc_apply   the filter: pass j takes the largest key below pass j - 1's; one pass then
//                 clears the source and counts what is kept.
// The per-slice connectivities (4, 8) run the same kernels with the links across slices switched off.
#include <algorithm>

#include "vh_internal.h"

#define CC_TPB 256
#define CC_TR 16
#define CC_TC 16
#define CC_TZ 24
#define CC_TILE (CC_TR * CC_TC * CC_TZ)   // 6144 voxels: 24 KiB of int32 labels in LDS
#define CC_LBITS 13                       // a tile-local index is < 2^13; a tile-local count is <= 6144 < 2^13
#define CC_LMASK ((1 << CC_LBITS) - 1)
#define CC_CLASSES 32                     // n_edges <= 31
#define CC_PICKS 8                        // keep_largest <= 8

static_assert(CC_TILE <= (1 << CC_LBITS), "a tile-local index and a tile-local count share an LDS word");

struct CcGeom {
    int R, C, Z;
    int tz;            // slices of a tile: Z where Z <= CC_TZ, else CC_TZ
    int ntc, ntz;      // tiles along C and Z
    int64_t V;
};

struct CcEdges {       // the class edges, by value
    uint32_t e[CC_CLASSES];
    int32_t n;
};

// ---- the union-find ----------------------------------------------------------------------------
// GLOBAL: the parent array is device memory that other workgroups change by atomics during the
// launch, so it is read at agent scope (past the CU's L1, which no other CU refreshes); else it is
// the workgroup's LDS.
template <bool GLOBAL>
__device__ __forceinline__ int cc_load(const int *p) {
    return GLOBAL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The root of x >= 0.  A value read late is an earlier parent: still an ancestor, so the walk still
// ends in x's set.
template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int *p, int x) {
    // bound: parent[y] < y on every step that continues, so at most x steps
    for (int guard = x; guard > 0; --guard) {
        const int y = cc_load<GLOBAL>(p + x);
        if (y == x) break;
        x = y;
    }
    return x;
}

// Unite the sets of a and b: the larger root takes the smaller as its parent by atomicMin.  Where the
// larger root had a parent by then, the atomicMin left it min(that parent, smaller root) and the
// displaced one of the two is united with the other in the next round.
template <bool GLOBAL>
__device__ __forceinline__ void cc_union(int *p, int a, int b) {
    // bound: a + b strictly decreases every round (find never increases; a failed atomicMin returns
    // a parent below a), so at most a + b + 1 rounds
    for (unsigned guard = (unsigned)a + (unsigned)b + 1u; guard > 0u; --guard) {
        a = cc_find<GLOBAL>(p, a);
        b = cc_find<GLOBAL>(p, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicMin(p + a, b);
        if (old == a) return;   // a was a root: linked
        a = old;
    }
}

// whether the step (dr, dc, dz) is a link of the connectivity that leads to a voxel before this one
// in index order: each link is united once, from its later end
template <bool PLANAR, bool DIAG>
__device__ __forceinline__ constexpr bool cc_back_link(int dr, int dc, int dz) {
    if (PLANAR && dz != 0) return false;
    const int a = (dr < 0 ? -dr : dr) + (dc < 0 ? -dc : dc) + (dz < 0 ? -dz : dz);
    if (a == 0 || (!DIAG && a != 1)) return false;
    return dr < 0 || (dr == 0 && (dc < 0 || (dc == 0 && dz < 0)));
}

// k_cc_local, grid (tiles, nb).  The tile's voxels in LDS in the volume's own order, (lr nc + lc) nz + lz
// with the tile's real extents: a partial tile is compact, every local index is a voxel of the volume,
// and the smallest local index of a set is its smallest linear index.
template <bool PLANAR, bool DIAG>
__global__ void __launch_bounds__(CC_TPB) k_cc_local(const uint8_t *__restrict__ src, int *__restrict__ root,
                                                     uint32_t *__restrict__ size, CcGeom g) {
    __shared__ int s_lab[CC_TILE];
    const int t = threadIdx.x;
    int tile = (int)blockIdx.x;
    const int z0 = (tile % g.ntz) * g.tz;
    tile /= g.ntz;
    const int c0 = (tile % g.ntc) * CC_TC;
    const int r0 = (tile / g.ntc) * CC_TR;
    const int nr = min(CC_TR, g.R - r0), nc = min(CC_TC, g.C - c0), nz = min(g.tz, g.Z - z0);
    const int n = nr * nc * nz;   // <= CC_TILE
    const int64_t sb = (int64_t)blockIdx.y * g.V;
    const uint8_t *a = src + sb;
    auto linear = [&](int i) {    // the study's linear index of local index i
        const int lz = i % nz, q = i / nz;
        return ((r0 + q / nc) * g.C + c0 + q % nc) * g.Z + z0 + lz;   // < V < 2^31
    };

    // (every loop over the tile's voxels below: at most CC_TILE / CC_TPB = 24 rounds)
    for (int i = t; i < n; i += CC_TPB) s_lab[i] = a[linear(i)] ? i : -1;
    __syncthreads();
    // The run axis: Z, or C for the per-slice connectivities.  A thread walks a line of the tile along
    // it and gives every voxel of a run the run's first voxel: the links along the axis cost no atomic.
    const int astr = PLANAR ? nz : 1, alen = PLANAR ? nc : nz, nlines = n / alen;
    for (int k = t; k < nlines; k += CC_TPB) {       // at most 384 / CC_TPB = 2 rounds
        const int base = PLANAR ? (k / nz) * nc * nz + k % nz : k * nz;
        int start = -1;
        for (int u = 0; u < alen; ++u) {             // at most CC_TZ = 24 steps
            const int i = base + u * astr;
            if (s_lab[i] < 0) {
                start = -1;
            } else {
                start = start < 0 ? i : start;
                s_lab[i] = start;
            }
        }
    }
    __syncthreads();
    for (int i = t; i < n; i += CC_TPB) {
        if (cc_load<false>(s_lab + i) < 0) continue;
        const int lz = i % nz, q = i / nz, lc = q % nc, lr = q / nc;
        // p, the voxel before this one along the axis: when p and p + d are set, the link d of this
        // voxel follows from p's and the two links along the axis, and is left out
        const bool prev = (PLANAR ? lc : lz) > 0 && cc_load<false>(s_lab + i - astr) >= 0;
#pragma unroll
        for (int dr = -1; dr <= 0; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc)
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    if (!cc_back_link<PLANAR, DIAG>(dr, dc, dz)) continue;
                    if (dr == 0 && (PLANAR ? dc == -1 : (dc == 0 && dz == -1))) continue;   // the axis: the runs
                    if (lr + dr < 0 || lc + dc < 0 || lc + dc >= nc || lz + dz < 0 || lz + dz >= nz) continue;
                    const int j = i + (dr * nc + dc) * nz + dz;
                    if (cc_load<false>(s_lab + j) < 0) continue;
                    if (prev && (PLANAR ? lc + dc : lz + dz) > 0 && cc_load<false>(s_lab + j - astr) >= 0) continue;
                    cc_union<false>(s_lab, i, j);
                }
    }
    __syncthreads();
    // every voxel takes its root (a neighbour's walk that reads the new value reads an ancestor)
    for (int i = t; i < n; i += CC_TPB)
        if (cc_load<false>(s_lab + i) >= 0)
            __hip_atomic_store(s_lab + i, cc_find<false>(s_lab, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    // the counts above the labels' bits, at the roots: an add of 2^13 leaves the low 13 bits alone,
    // and only a root's word (its own label) is added to
    for (int i = t; i < n; i += CC_TPB) {
        const int v = cc_load<false>(s_lab + i);
        if (v >= 0) atomicAdd(s_lab + (v & CC_LMASK), 1 << CC_LBITS);
    }
    __syncthreads();
    for (int i = t; i < n; i += CC_TPB) {
        const int v = s_lab[i];
        const int64_t e = sb + linear(i);
        const int rt = v & CC_LMASK;
        root[e] = v < 0 ? -1 : linear(rt);
        size[e] = (v >= 0 && rt == i) ? (uint32_t)(v >> CC_LBITS) : 0u;
    }
}

// k_cc_merge, grid (voxels / CC_TPB, nb): a set voxel next to a face of its tile unites with its
// earlier neighbours in other tiles.
template <bool PLANAR, bool DIAG>
__global__ void __launch_bounds__(CC_TPB) k_cc_merge(int *root, CcGeom g) {
    const int64_t e64 = (int64_t)blockIdx.x * CC_TPB + threadIdx.x;
    if (e64 >= g.V) return;
    const int e = (int)e64;
    const int z = e % g.Z, q = e / g.Z, c = q % g.C, r = q / g.C;
    const int lr = r % CC_TR, lc = c % CC_TC, lz = z % g.tz;
    bool face = lr == 0 || lc == 0 || (DIAG && lc == CC_TC - 1);
    if (!PLANAR && g.ntz > 1) face = face || lz == 0 || (DIAG && lz == g.tz - 1);
    if (!face) return;
    int *p = root + (int64_t)blockIdx.y * g.V;
    if (cc_load<true>(p + e) < 0) return;
    // as in k_cc_local: with the voxel before this one along the run axis and that voxel's neighbour by
    // d both set, the link d follows from theirs (made here or in k_cc_local) and the links along the axis
    const int astr = PLANAR ? g.Z : 1;
    const bool prev = (PLANAR ? c : z) > 0 && cc_load<true>(p + e - astr) >= 0;
#pragma unroll
    for (int dr = -1; dr <= 0; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                if (!cc_back_link<PLANAR, DIAG>(dr, dc, dz)) continue;
                const int r2 = r + dr, c2 = c + dc, z2 = z + dz;
                if (r2 < 0 || c2 < 0 || c2 >= g.C || z2 < 0 || z2 >= g.Z) continue;
                if (r2 / CC_TR == r / CC_TR && c2 / CC_TC == c / CC_TC && z2 / g.tz == z / g.tz) continue;   // k_cc_local's
                const int j = (r2 * g.C + c2) * g.Z + z2;
                if (cc_load<true>(p + j) < 0) continue;
                const bool axis = dr == 0 && (PLANAR ? dc == -1 : (dc == 0 && dz == -1));
                if (!axis && prev && (PLANAR ? c2 : z2) > 0 && cc_load<true>(p + j - astr) >= 0) continue;
                cc_union<true>(p, e, j);
            }
}

// k_cc_flatten, grid (voxels / CC_TPB, nb).  Nothing unites here: a walk that meets a root another
// thread has just stored meets an ancestor.  size[] holds the tile-local counts at the tile-local
// roots and 0 elsewhere; a component's root is the tile-local root of its own tile, so its entry starts
// at its own tile's count and takes the others'.  Only roots' entries are added to, and no thread reads
// one but the root's own, which adds nothing.
__global__ void __launch_bounds__(CC_TPB) k_cc_flatten(int *root, uint32_t *size, int64_t V) {
    const int64_t e64 = (int64_t)blockIdx.x * CC_TPB + threadIdx.x;
    if (e64 >= V) return;
    const int e = (int)e64;
    int *p = root + (int64_t)blockIdx.y * V;
    uint32_t *sz = size + (int64_t)blockIdx.y * V;
    if (p[e] < 0) return;
    const int rt = cc_find<true>(p, e);
    __hip_atomic_store(p + e, rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t s = sz[e];
    if (s && rt != e) atomicAdd(sz + rt, s);
}

__device__ __forceinline__ unsigned long long cc_key(uint32_t size, int root) {
    return ((unsigned long long)size << 32) | (unsigned long long)(~(uint32_t)root);
}

// k_cc_summary, grid (voxels / CC_TPB, nb): the size of every voxel's component onto the voxel (a
// root's entry is read by others and is not written), and the study's summary: stats[0] n_set, [1]
// n_comp, [2] the largest key (0: no component), counts[k] = {components of class k, their voxels}.
__global__ void __launch_bounds__(CC_TPB) k_cc_summary(const int *__restrict__ root, uint32_t *size, int64_t V,
                                                       CcEdges ed, unsigned long long *counts,
                                                       unsigned long long *stats) {
    __shared__ unsigned long long s_cnt[2 * CC_CLASSES];
    __shared__ unsigned long long s_best;
    __shared__ uint32_t s_n[2];
    const int t = threadIdx.x;
    if (t < 2 * CC_CLASSES) s_cnt[t] = 0ull;
    if (t == 64) s_best = 0ull;
    if (t >= 66 && t < 68) s_n[t - 66] = 0u;
    __syncthreads();
    const int64_t e64 = (int64_t)blockIdx.x * CC_TPB + t;
    const int64_t sb = (int64_t)blockIdx.y;
    const int rt = e64 < V ? root[sb * V + e64] : -1;
    const unsigned long long set = __ballot(rt >= 0);
    if (set && (t & 63) == 0) atomicAdd(&s_n[0], (uint32_t)__popcll(set));
    if (rt >= 0) {
        uint32_t *sz = size + sb * V;
        const uint32_t s = sz[rt];
        if (rt != (int)e64) {
            sz[e64] = s;
        } else {
            int k = 0;
            for (int i = 0; i < ed.n; ++i) k += ed.e[i] <= s ? 1 : 0;   // bound: n_edges <= 31
            atomicAdd(&s_cnt[2 * k], 1ull);
            atomicAdd(&s_cnt[2 * k + 1], (unsigned long long)s);
            atomicAdd(&s_n[1], 1u);
            atomicMax(&s_best, cc_key(s, rt));
        }
    }
    __syncthreads();
    unsigned long long *cq = counts + sb * 2 * (ed.n + 1), *sq = stats + sb * 4;
    if (t < 2 * (ed.n + 1) && s_cnt[t]) atomicAdd(&cq[t], s_cnt[t]);
    if (t == 64 && s_n[0]) atomicAdd(&sq[0], (unsigned long long)s_n[0]);
    if (t == 65 && s_n[1]) atomicAdd(&sq[1], (unsigned long long)s_n[1]);
    if (t == 66 && s_best) atomicMax(&sq[2], s_best);
}

// k_cc_pick, grid (voxels / CC_TPB, nb): pass j of the studies with keep_largest > j: the largest key
// below pass j - 1's pick (every key, for pass 0) into picks[j].  Keys differ (the roots do); a study
// with fewer components leaves 0.
__global__ void __launch_bounds__(CC_TPB) k_cc_pick(const int *__restrict__ root, const uint32_t *__restrict__ size,
                                                    int64_t V, const int32_t *__restrict__ keep, int j,
                                                    unsigned long long *picks) {
    __shared__ unsigned long long s_best;
    const int64_t sb = (int64_t)blockIdx.y;
    if (keep[sb] <= j) return;   // (uniform over the workgroup)
    const int t = threadIdx.x;
    if (t == 0) s_best = 0ull;
    __syncthreads();
    const int64_t e64 = (int64_t)blockIdx.x * CC_TPB + t;
    if (e64 < V && root[sb * V + e64] == (int)e64) {
        const unsigned long long key = cc_key(size[sb * V + e64], (int)e64);
        if (j == 0 || key < picks[sb * CC_PICKS + j - 1]) atomicMax(&s_best, key);
    }
    __syncthreads();
    if (t == 0 && s_best) atomicMax(&picks[sb * CC_PICKS + j], s_best);
}

// k_cc_apply, grid (voxels / CC_TPB, nb): a voxel of S stays when its component has min_size voxels
// and, with keep_largest = k > 0, a key at or above the k-th pick (0 where the study has fewer than k
// components: all pass); every other voxel of the source is cleared.  kept[q] = {components, voxels}.
__global__ void __launch_bounds__(CC_TPB) k_cc_apply(uint8_t *src, const int *__restrict__ root,
                                                     const uint32_t *__restrict__ size, int64_t V,
                                                     const uint32_t *__restrict__ min_size,
                                                     const int32_t *__restrict__ keep,
                                                     const unsigned long long *__restrict__ picks,
                                                     unsigned long long *kept) {
    __shared__ uint32_t s_n[2];
    const int t = threadIdx.x;
    if (t < 2) s_n[t] = 0u;
    __syncthreads();
    const int64_t sb = (int64_t)blockIdx.y;
    const int64_t e64 = (int64_t)blockIdx.x * CC_TPB + t;
    const int rt = e64 < V ? root[sb * V + e64] : -1;
    bool stays = false;
    if (rt >= 0) {
        const uint32_t s = size[sb * V + e64];
        const int k = keep[sb];
        stays = s >= min_size[sb] && (k == 0 || cc_key(s, rt) >= picks[sb * CC_PICKS + k - 1]);
        if (!stays) src[sb * V + e64] = (uint8_t)0;
    }
    const unsigned long long nv = __ballot(stays), nc = __ballot(stays && rt == (int)e64);
    if ((t & 63) == 0) {
        if (nv) atomicAdd(&s_n[1], (uint32_t)__popcll(nv));
        if (nc) atomicAdd(&s_n[0], (uint32_t)__popcll(nc));
    }
    __syncthreads();
    if (t < 2 && s_n[t]) atomicAdd(&kept[sb * 2 + t], (unsigned long long)s_n[t]);
}

// ---- the launchers -------------------------------------------------------------------------------
static CcGeom cc_geom(const vh_batch *b) {
    CcGeom g;
    g.R = (int)b->R;
    g.C = (int)b->C;
    g.Z = (int)b->Z;
    g.V = b->V;
    g.tz = (int)std::min<int64_t>(b->Z, CC_TZ);
    g.ntc = (g.C + CC_TC - 1) / CC_TC;
    g.ntz = (g.Z + g.tz - 1) / g.tz;
    return g;
}

// grid y is the study; the tiles and the voxel blocks are far below 2^31 (V < 2^31: check_dims)
bool vh_cc_takes(const vh_batch *b) { return b->nb <= 65535 && b->V < ((int64_t)1 << 31); }

template <bool PLANAR, bool DIAG>
static void cc_label(vh_batch *b, const uint8_t *src, int *root, uint32_t *size) {
    hipStream_t st = b->stream;
    const CcGeom g = cc_geom(b);
    const int64_t tiles = (int64_t)((g.R + CC_TR - 1) / CC_TR) * g.ntc * g.ntz;
    const dim3 gt((unsigned)tiles, (unsigned)b->nb, 1);
    const dim3 gv((unsigned)((b->V + CC_TPB - 1) / CC_TPB), (unsigned)b->nb, 1);
    k_cc_local<PLANAR, DIAG><<<gt, CC_TPB, 0, st>>>(src, root, size, g);
    VH_CHECK_LAUNCH();
    if (tiles > 1) {
        k_cc_merge<PLANAR, DIAG><<<gv, CC_TPB, 0, st>>>(root, g);
        VH_CHECK_LAUNCH();
        k_cc_flatten<<<gv, CC_TPB, 0, st>>>(root, size, b->V);
        VH_CHECK_LAUNCH();
    }
}

void vh_cc_launch(vh_batch *b, const uint8_t *src, int conn, const uint32_t *edges, int n_edges, int *root,
                  uint32_t *size, unsigned long long *d_counts, unsigned long long *d_stats) {
    hipStream_t st = b->stream;
    CcEdges ed{};
    ed.n = n_edges;
    std::copy(edges, edges + n_edges, ed.e);
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t)b->nb * 2 * (n_edges + 1), st));
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * (size_t)b->nb * 4, st));
    // the algorithmic bytes: the source read, the root and the size maps written
    ScopedKTimer tm(b, "comp_b", 9.0 * (double)b->nb * (double)b->V);
    switch (conn) {
        case 4: cc_label<true, false>(b, src, root, size); break;
        case 8: cc_label<true, true>(b, src, root, size); break;
        case 6: cc_label<false, false>(b, src, root, size); break;
        default: cc_label<false, true>(b, src, root, size); break;
    }
    const dim3 gv((unsigned)((b->V + CC_TPB - 1) / CC_TPB), (unsigned)b->nb, 1);
    k_cc_summary<<<gv, CC_TPB, 0, st>>>(root, size, b->V, ed, d_counts, d_stats);
    VH_CHECK_LAUNCH();
}

void vh_cc_filter_launch(vh_batch *b, uint8_t *src, const int *root, const uint32_t *size, const uint32_t *d_min,
                         const int32_t *d_keep, int kmax, unsigned long long *d_picks, unsigned long long *d_kept) {
    hipStream_t st = b->stream;
    HIP_TRY(hipMemsetAsync(d_picks, 0, sizeof(unsigned long long) * (size_t)b->nb * CC_PICKS, st));
    HIP_TRY(hipMemsetAsync(d_kept, 0, sizeof(unsigned long long) * (size_t)b->nb * 2, st));
    // the algorithmic bytes: the source read and written
    ScopedKTimer tm(b, "comp_b", 2.0 * (double)b->nb * (double)b->V);
    const dim3 gv((unsigned)((b->V + CC_TPB - 1) / CC_TPB), (unsigned)b->nb, 1);
    for (int j = 0; j < kmax; ++j) {   // kmax <= CC_PICKS
        k_cc_pick<<<gv, CC_TPB, 0, st>>>(root, size, b->V, d_keep, j, d_picks);
        VH_CHECK_LAUNCH();
    }
    k_cc_apply<<<gv, CC_TPB, 0, st>>>(src, root, size, b->V, d_min, d_keep, d_picks, d_kept);
    VH_CHECK_LAUNCH();
}
