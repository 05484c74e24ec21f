// register.hip -- the rigid integer-voxel alignment of the proton to the xenon image of a resident
// batch by mutual information (vh_batch_register, vh_batch_shift); the spec is in include/vent_hip.h.
// Four kernels: the code pass (two images -> 32-level byte codes), the joint histogram of every shift
// of the search window (the hot path), the score of every histogram in double, and the shift itself.
// Every count is an exact integer; only the score is floating point.
#include <algorithm>

#include "vh_internal.h"

#define RG_TPB 256
#define RG_NW 8                     // waves of a joint-histogram workgroup: a shift each per round
#define RG_NC 2                     // copies of a wave's histogram: lane l counts in copy l % RG_NC
#define RG_HP 1025                  // words between the copies: the copies of a bin lie on different banks
#define RG_JTPB (64 * RG_NW)
#define RG_LDS_MAX (156 * 1024)     // histograms and both code tiles: inside the CU's 160 KiB
#define RG_LDS_PLAIN (64 * 1024)    // above it the launch needs MaxDynamicSharedMemorySize

// ---- codes (rg_in_f, rg_code, RG_INVALID: vh_internal.h, shared with register_maps.hip) ----------------
// cp / cx [nb][V] = the codes of the proton and of the HPvent; maxb [2][nb] the bit patterns of their
// maxima over F (k_seg_max).  A study whose maximum is not > 0 is unregistrable: its codes are never
// read, and are written as invalid.  grid (blocks, nb)
__global__ void __launch_bounds__(RG_TPB) k_reg_codes(const float *__restrict__ p, const float *__restrict__ x,
                                                      int64_t V, const uint32_t *__restrict__ maxb, int64_t nb,
                                                      uint8_t *__restrict__ cp, uint8_t *__restrict__ cx) {
    const float pm = __uint_as_float(maxb[blockIdx.y]), xm = __uint_as_float(maxb[nb + blockIdx.y]);
    const bool ok = pm > 0.0f && xm > 0.0f;
    const float ps = __fdiv_rn(256.0f, pm), xs = __fdiv_rn(256.0f, xm);
    const int64_t base = (int64_t)blockIdx.y * V;
    const int64_t step = (int64_t)gridDim.x * RG_TPB;
    for (int64_t i = blockIdx.x * (int64_t)RG_TPB + threadIdx.x; i < V; i += step) {
        cp[base + i] = (uint8_t)(ok ? rg_code(p[base + i], ps) : RG_INVALID);
        cx[base + i] = (uint8_t)(ok ? rg_code(x[base + i], xs) : RG_INVALID);
    }
}

// ---- the joint histograms -------------------------------------------------------------------------
// One workgroup = one (study, tile of TR x TC x TZ xenon voxels, chunk of shifts): grid (tiles, chunks,
// nb).  The tile's codes are staged in LDS once and serve every shift of the chunk:
//   ps   the proton codes of the tile and its halo, [TR + 2 Sr][PC][PZ] bytes, PC = TC + 2 Sc and
//        PZ = TZ + 2 Sz; a cell outside the volume is invalid (255)
//   xs   the xenon codes, [TR][PC][PZ] bytes: the same column and slice pitch, the halo cells and
//        whatever of the tile hangs over the volume's edge invalid
// With equal pitches the proton partner of xenon byte i under shift (dr, dc, dz) is proton byte
// i + ((Sr + dr) PC + dc) PZ + dz whatever i's row, column and slice are: the inner loop has no index
// arithmetic.  An invalid xenon byte (a halo cell) may point outside ps -- into the margins of M bytes
// allocated before and after it -- and is skipped whatever it finds there.
//
// A lane takes four consecutive bytes at a time: one aligned word of xs, two aligned words of ps funnel-
// shifted by the shift's byte phase (uniform in the wave).  A wave takes one shift of the chunk per
// round and walks the whole tile, counting into its own histogram with LDS adds; the waves never share
// a counter.  An image puts most of a wave into a few bins and adds to one LDS word go one after the
// other, so a wave keeps RG_NC copies of its 4 KiB histogram, lane l counting in copy l % RG_NC, copy j at
// word RG_HP j.  Pairs of bin (0, 0) -- the background of both images, most of a real study -- are not
// added: every lane counts its own in a register and the wave adds the sum once per shift, so the
// hottest bin costs no LDS add at all.  After its walk the wave adds its occupied bins to the global
// histogram of (study, shift) (zeroed by the caller; the tiles of a study meet there) and clears them.
struct RgGeom {
    int R, C, Z;
    int Sr, Sc, Sz;
    int TR, TC, TZ;
    int PC, PZ;
    int ntr, ntc, ntz;   // tiles along each axis
    int ns, chunk;       // shifts; shifts per workgroup
    int xn4;             // words of xs
    int M;               // margin bytes of ps, a multiple of 4
    int pn4;             // words of ps, margins included
};

__global__ void __launch_bounds__(RG_JTPB) k_reg_joint(const uint8_t *__restrict__ cp, const uint8_t *__restrict__ cx,
                                                       int64_t V, const uint32_t *__restrict__ maxb, int64_t nb,
                                                       RgGeom g, uint32_t *__restrict__ hist,
                                                       unsigned long long *ks) {
    extern __shared__ uint32_t s_rg[];
    kst_begin(ks);
    const float pm = __uint_as_float(maxb[blockIdx.z]), xm = __uint_as_float(maxb[nb + blockIdx.z]);
    if (pm > 0.0f && xm > 0.0f) {   // (the whole workgroup: the maxima are per study)
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        uint32_t *s_h = s_rg + wave * (RG_NC * RG_HP);
        uint32_t *mine = s_h + (lane % RG_NC) * RG_HP;
        uint32_t *s_x = s_rg + RG_NW * RG_NC * RG_HP;
        uint32_t *s_p = s_x + g.xn4;
        uint8_t *xb = reinterpret_cast<uint8_t *>(s_x);
        uint8_t *pb = reinterpret_cast<uint8_t *>(s_p) + g.M;   // cell (0, 0, 0) of ps
        int t = (int)blockIdx.x;
        const int tz = t % g.ntz; t /= g.ntz;
        const int tc = t % g.ntc;
        const int tr = t / g.ntc;
        const int r0 = tr * g.TR, c0 = tc * g.TC, z0 = tz * g.TZ;
        const int PC = g.PC, PZ = g.PZ;
        const uint8_t *gp = cp + (int64_t)blockIdx.z * V, *gx = cx + (int64_t)blockIdx.z * V;

        for (int i = tid; i < RG_NW * RG_NC * RG_HP; i += RG_JTPB) s_rg[i] = 0u;
        // the last two words of xs hold the bytes past the tile: invalid (xn4 >= 2; the staging follows a barrier)
        if (tid < 2) s_x[g.xn4 - 1 - tid] = 0xffffffffu;
        __syncthreads();
        // staging, a thread per (row, column) pencil of PZ slices
        for (int q = tid; q < g.TR * PC; q += RG_JTPB) {
            const int rl = q / PC, cl = q - rl * PC;
            const int r = r0 + rl, c = c0 + cl - g.Sc;
            const bool in = r < g.R && cl >= g.Sc && cl < g.Sc + g.TC && c < g.C;
            const uint8_t *src = gx + ((int64_t)r * g.C + c) * g.Z;
            uint8_t *dst = xb + q * PZ;
            for (int zl = 0; zl < PZ; ++zl) {
                const int z = z0 + zl - g.Sz;
                dst[zl] = (in && zl >= g.Sz && zl < g.Sz + g.TZ && z < g.Z) ? src[z] : (uint8_t)RG_INVALID;
            }
        }
        for (int q = tid; q < (g.TR + 2 * g.Sr) * PC; q += RG_JTPB) {
            const int rl = q / PC, cl = q - rl * PC;
            const int r = r0 + rl - g.Sr, c = c0 + cl - g.Sc;
            const bool in = r >= 0 && r < g.R && c >= 0 && c < g.C;
            const uint8_t *src = gp + ((int64_t)r * g.C + c) * g.Z;
            uint8_t *dst = pb + q * PZ;
            for (int zl = 0; zl < PZ; ++zl) {
                const int z = z0 + zl - g.Sz;
                dst[zl] = (in && z >= 0 && z < g.Z) ? src[z] : (uint8_t)RG_INVALID;
            }
        }
        __syncthreads();

        const int sa = (int)blockIdx.y * g.chunk, sb = min(sa + g.chunk, g.ns);
        const int wr = 2 * g.Sr + 1, wc = 2 * g.Sc + 1;
        uint32_t *hs = hist + (size_t)blockIdx.z * (size_t)g.ns * RG_BINS;
        for (int s = sa + wave; s < sb; s += RG_NW) {   // (no barrier below: a wave's histogram is its own)
            int q = s;
            const int dc = q % wc - g.Sc; q /= wc;
            const int dr = q % wr - g.Sr;
            const int dz = q / wr - g.Sz;
            // the byte of ps (margin included) that pairs with byte 0 of xs: never negative
            const int B = g.M + ((g.Sr + dr) * PC + dc) * PZ + dz;
            const uint32_t *pw = s_p + (B >> 2);
            const uint32_t ph = (uint32_t)(B & 3) * 8u;
            uint32_t n00 = 0u;
            // the words of the next step are read before this step's are counted: an LDS read waits behind
            // the adds every wave of the workgroup has queued
            int i = lane;
            uint32_t xw = 0xffffffffu, lo = 0u, hi = 0u;
            if (i < g.xn4) { xw = s_x[i]; lo = pw[i]; hi = pw[i + 1]; }
            while (i < g.xn4) {
                const uint32_t cx4 = xw, cp4 = __funnelshift_r(lo, hi, ph);
                i += 64;
                if (i < g.xn4) { xw = s_x[i]; lo = pw[i]; hi = pw[i + 1]; }
                // a byte of either is a code 0..31 or 255.  t: the OR of the pair's codes, 0 for a pair of bin
                // (0, 0), 1..31 for any other valid pair, above for an invalid one
                const uint32_t t = cx4 | cp4;
                n00 += (uint32_t)__popc(~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u);   // its zero bytes
                // the byte offsets 4 (32 a + b) of bytes 0 and 2, and of 1 and 3, as 16-bit fields
                const uint32_t e = ((cp4 & 0x00ff00ffu) << 7) + ((cx4 & 0x00ff00ffu) << 2);
                const uint32_t o = (((cp4 >> 8) & 0x00ff00ffu) << 7) + (((cx4 >> 8) & 0x00ff00ffu) << 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t tj = (t >> (8 * j)) & 0xffu;
                    const uint32_t at = (((j & 1) ? o : e) >> (16 * (j >> 1))) & 0xffffu;
                    if (tj - 1u < 31u) atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(mine) + at), 1u);
                }
            }
            for (int off = 32; off > 0; off >>= 1) n00 += __shfl_xor(n00, off, 64);
            // (a wave's LDS operations complete in program order: the adds above precede these reads)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t *out = hs + (size_t)s * RG_BINS;
#pragma unroll 4
            for (int k = lane; k < RG_BINS; k += 64) {
                uint32_t n = k == 0 ? n00 : 0u;
#pragma unroll
                for (int c = 0; c < RG_NC; ++c) {
                    const uint32_t v = s_h[c * RG_HP + k];
                    if (v) s_h[c * RG_HP + k] = 0u;
                    n += v;
                }
                if (n) atomicAdd(out + k, n);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
    kst_end(ks);
}

static size_t rg_lds_bytes(const RgGeom &g) {
    return sizeof(uint32_t) * ((size_t)RG_NW * RG_NC * RG_HP + g.xn4 + g.pn4);
}

static void rg_fill(RgGeom &g) {
    g.PC = g.TC + 2 * g.Sc;
    g.PZ = g.TZ + 2 * g.Sz;
    const int xn = g.TR * g.PC * g.PZ;
    g.xn4 = (xn + 3) / 4 + 1;   // (a whole invalid word closes it: the kernel writes it before staging)
    // byte i of xs pairs with a byte of ps between i - (Sc PZ + Sz) and i + 2 Sr PC PZ + Sc PZ + Sz; the
    // second word of a funnel shift lies up to 7 bytes further
    g.M = ((g.Sc * g.PZ + g.Sz + 3) / 4) * 4;
    const int pn = (g.TR + 2 * g.Sr) * g.PC * g.PZ;
    g.pn4 = (g.M + std::max(pn, 4 * g.xn4 + 2 * g.Sr * g.PC * g.PZ) + g.M + 8 + 3) / 4;
}

// The tile: of the candidates (rows up to 8, columns up to 128, slices up to 32, each halved down
// to 1) the one with the most xenon voxels whose codes fit beside the histograms -- a study then takes the
// fewest workgroups, its occupied bins reach the global histogram the fewest times, and the halo is the
// smallest share of the staging; among equals the one with the most rows, then columns.
static RgGeom rg_geometry(const vh_batch *b, const int32_t search[3]) {
    RgGeom g;
    g.R = (int)b->R; g.C = (int)b->C; g.Z = (int)b->Z;
    g.Sr = search[0]; g.Sc = search[1]; g.Sz = search[2];
    int best[3] = {1, 1, 1};
    long bv = -1;
    for (int tr = std::min(g.R, 8);; tr = (tr + 1) / 2) {
        for (int tc = std::min(g.C, 128);; tc = (tc + 1) / 2) {
            for (int tz = std::min(g.Z, 32);; tz = (tz + 1) / 2) {
                g.TR = tr; g.TC = tc; g.TZ = tz;
                rg_fill(g);
                const long v = (long)tr * tc * tz;
                if (rg_lds_bytes(g) <= RG_LDS_MAX && v > bv) { bv = v; best[0] = tr; best[1] = tc; best[2] = tz; }
                if (tz == 1) break;
            }
            if (tc == 1) break;
        }
        if (tr == 1) break;
    }
    g.TR = best[0]; g.TC = best[1]; g.TZ = best[2];
    rg_fill(g);
    g.ntr = (g.R + g.TR - 1) / g.TR;
    g.ntc = (g.C + g.TC - 1) / g.TC;
    g.ntz = (g.Z + g.TZ - 1) / g.TZ;
    g.ns = (2 * g.Sr + 1) * (2 * g.Sc + 1) * (2 * g.Sz + 1);
    // shifts per workgroup: all of them where the tiles alone fill the device (the staging is paid once),
    // else chunks of whole rounds until there are about 2048 workgroups
    const int64_t tiles = (int64_t)g.ntr * g.ntc * g.ntz * b->nb;
    const int64_t rounds = (g.ns + RG_NW - 1) / RG_NW;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(rounds, (2048 + tiles - 1) / tiles));
    g.chunk = (int)((rounds + want - 1) / want) * RG_NW;
    return g;
}

bool vh_register_takes(const vh_batch *b) {   // grid z, grid x
    return b->nb <= 65535 && b->R * b->C * b->Z < ((int64_t)1 << 31);   // (a tile holds a voxel at least)
}

void vh_register_launch(vh_batch *b, const float *proton, const float *hp, const int32_t search[3],
                        uint32_t *d_maxb, uint8_t *d_cp, uint8_t *d_cx, uint32_t *d_hist, double *d_score) {
    const size_t nb = (size_t)b->nb;
    const RgGeom g = rg_geometry(b, search);
    const size_t lds = rg_lds_bytes(g);
    if (lds > RG_LDS_MAX) throw VhError{VH_ERR_ARG, "register: the tile does not fit"};
    HIP_TRY(hipMemsetAsync(d_maxb, 0, sizeof(uint32_t) * 2 * nb, b->stream));
    vh_seg_max_launch(b, proton, d_maxb);
    vh_seg_max_launch(b, hp, d_maxb + nb);
    {
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((b->V + RG_TPB * 8 - 1) / (RG_TPB * 8), 256));
        ScopedKTimer tm(b, "register_codes_b", 10.0 * (double)nb * (double)b->V);
        k_reg_codes<<<dim3((unsigned)blocks, (unsigned)nb, 1), RG_TPB, 0, b->stream>>>(proton, hp, b->V, d_maxb, b->nb,
                                                                                      d_cp, d_cx);
        VH_CHECK_LAUNCH();
    }
    HIP_TRY(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * nb * (size_t)g.ns * RG_BINS, b->stream));
    {
        if (lds > RG_LDS_PLAIN) vh_set_max_lds((const void *)k_reg_joint, RG_LDS_MAX);
        const dim3 grid((unsigned)(g.ntr * g.ntc * g.ntz), (unsigned)((g.ns + g.chunk - 1) / g.chunk), (unsigned)nb);
        ScopedKTimer tm(b, "register_b", 2.0 * (double)nb * (double)b->V, true);
        k_reg_joint<<<grid, RG_JTPB, lds, b->stream>>>(d_cp, d_cx, b->V, d_maxb, b->nb, g, d_hist, tm.stamp());
        VH_CHECK_LAUNCH();
    }
    vh_register_score_launch(b, d_hist, d_maxb, g.ns, d_score);
}

// ---- the score ------------------------------------------------------------------------------------
// One wave = one (study, shift): grid (ceil(ns / 4), nb), four waves a workgroup.  Step t of 16 reads
// bins 64 t .. 64 t + 63: lane l holds J[a][b] with a = 2 t + l / 32 and b = l % 32.  The row sum
// closes inside each half wave, the column sums add up over the steps and then across the halves; all
// are exact integers below 2^32.  mi = (1 / n) sum over J > 0 of J log((J n) / (Ja Jb)) in double: both
// products are exact (below 2^53), so equal products give a quotient of exactly 1.0 and a term of
// exactly 0.0.  NaN for an unregistrable study.
__global__ void __launch_bounds__(RG_TPB) k_reg_score(const uint32_t *__restrict__ hist,
                                                      const uint32_t *__restrict__ maxb, int64_t nb, int ns,
                                                      double *__restrict__ score, unsigned long long *ks) {
    kst_begin(ks);
    const int lane = threadIdx.x & 63;
    const int s = (int)blockIdx.x * (RG_TPB / 64) + (threadIdx.x >> 6);
    if (s < ns) {   // (wave-uniform)
        const float pm = __uint_as_float(maxb[blockIdx.y]), xm = __uint_as_float(maxb[nb + blockIdx.y]);
        const size_t at = (size_t)blockIdx.y * (size_t)ns + (size_t)s;
        if (!(pm > 0.0f && xm > 0.0f)) {
            if (lane == 0) score[at] = __longlong_as_double(0x7ff8000000000000ll);
        } else {
            const uint32_t *J = hist + at * RG_BINS;
            uint32_t j[16], ja[16];
            unsigned long long jb = 0ull;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                j[t] = J[64 * t + lane];
                jb += j[t];
                unsigned long long r = j[t];
                for (int off = 16; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
                ja[t] = (uint32_t)r;   // (a row sum is at most the voxels of a study: < 2^31)
            }
            jb += __shfl_xor(jb, 32, 64);
            unsigned long long n = jb;   // every lane of a half holds one column: the half's sum is n
            for (int off = 16; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j[t]) {
                    const double num = (double)j[t] * (double)n;
                    const double den = (double)ja[t] * (double)jb;
                    acc += (double)j[t] * log(num / den);
                }
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (lane == 0) score[at] = n ? acc / (double)n : 0.0;
        }
    }
    kst_end(ks);
}

void vh_register_score_launch(vh_batch *b, const uint32_t *d_hist, const uint32_t *d_maxb, int ns, double *d_score) {
    const dim3 grid((unsigned)((ns + RG_TPB / 64 - 1) / (RG_TPB / 64)), (unsigned)b->nb, 1);
    ScopedKTimer tm(b, "register_score_b", 4.0 * RG_BINS * (double)b->nb * (double)ns, true);
    k_reg_score<<<grid, RG_TPB, 0, b->stream>>>(d_hist, d_maxb, b->nb, ns, d_score, tm.stamp());
    VH_CHECK_LAUNCH();
}

// ---- the shift ------------------------------------------------------------------------------------
// dst(v) = src(v + s) where v + s is inside the volume, else 0, s = shift[study]: grid (blocks, nb)
template <class T>
__global__ void __launch_bounds__(RG_TPB) k_reg_shift(const T *__restrict__ src, T *__restrict__ dst, int64_t R, int64_t C,
                                                      int64_t Z, const int32_t *__restrict__ shift,
                                                      unsigned long long *ks) {
    kst_begin(ks);
    const int64_t V = R * C * Z;   // (below 2^31, like every volume of a batch: the index arithmetic is 32-bit)
    const uint32_t CZ = (uint32_t)(C * Z), Z32 = (uint32_t)Z;
    const int32_t *s = shift + 3 * (int64_t)blockIdx.y;
    const int32_t dr = s[0], dc = s[1], dz = s[2];
    const int64_t off = ((int64_t)dr * C + dc) * Z + dz;
    const T *xs = src + (int64_t)blockIdx.y * V;
    T *ys = dst + (int64_t)blockIdx.y * V;
    const uint32_t step = gridDim.x * RG_TPB;
    for (uint32_t v = blockIdx.x * RG_TPB + threadIdx.x; v < (uint32_t)V; v += step) {
        const uint32_t r = v / CZ, rem = v - r * CZ;
        const uint32_t c = rem / Z32, z = rem - c * Z32;
        const int32_t r2 = (int32_t)r + dr, c2 = (int32_t)c + dc, z2 = (int32_t)z + dz;
        const bool in = r2 >= 0 && r2 < (int32_t)R && c2 >= 0 && c2 < (int32_t)C && z2 >= 0 && z2 < (int32_t)Z;
        ys[v] = in ? xs[(int64_t)v + off] : (T)0;
    }
    kst_end(ks);
}

template <class T>
static void rg_shift_launch(vh_batch *b, const T *src, T *dst, const int32_t *d_shift) {
    if (b->nb > 65535) throw VhError{VH_ERR_ARG, "shift: more than 65535 studies"};   // (grid y)
    // 32 voxels per thread: with 4 (384 workgroups per study of the bench batch) the shift took 1.14 ms,
    // workgroups ending as soon as they had started (the sweeps of segment.hip met the same)
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((b->V + RG_TPB * 32 - 1) / (RG_TPB * 32), 64));
    // stamped: the kernel follows the shifts' upload on the stream (see vh_mask_paint_launch)
    ScopedKTimer tm(b, "shift_b", 2.0 * sizeof(T) * (double)b->nb * (double)b->V, true);
    k_reg_shift<T><<<dim3((unsigned)blocks, (unsigned)b->nb, 1), RG_TPB, 0, b->stream>>>(src, dst, b->R, b->C, b->Z,
                                                                                       d_shift, tm.stamp());
    VH_CHECK_LAUNCH();
}

void vh_shift_launch_f32(vh_batch *b, const float *src, float *dst, const int32_t *d_shift) {
    rg_shift_launch<float>(b, src, dst, d_shift);
}
void vh_shift_launch_u8(vh_batch *b, const uint8_t *src, uint8_t *dst, const int32_t *d_shift) {
    rg_shift_launch<uint8_t>(b, src, dst, d_shift);
}
