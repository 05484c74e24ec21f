// export.hip -- the rendering steps that follow the hot path, on device.
//
//  * exportDICOM (Vent_Analysis.py:381-397): BW = uint8(normalize(|N4HPvent|) * 255) in float32,
//    RGB = (BW*(defect==0) + 255*(defect==1), BW*(defect==0), BW*(defect==0)).  Written
//    slice-major [Z][R][C][3]: the frame order of np.transpose(RGB, (2,0,1,3)) (:393) and, frame
//    by frame, the RGB[:,:,i,:] images of the PACS branch (:410-411).
//  * screenShot (Vent_Analysis.py:458-500): the 7-row montage (blank, blank, proton, HPvent,
//    N4 + mask border, N4 + defects, N4 + parula CI) over the mask's bounding box, each panel
//    normalised over the crop, stored as uint8(IMAGE * 255) with IMAGE in float64.
//
// Both are per-voxel maps: HBM-bound streaming (overlay: 4 B N4 + 1 B defect in, 3 B out per
// voxel) with the volume min/max as an order-free integer reduction (float bits of |x| are
// monotone), so every output byte is bit-identical to numpy's.
#include "vh_internal.h"

#define OV_COLS 64     // columns per overlay block (one wave's worth of output words per slice)
#define OV_ZC 64       // slices per overlay block
#define OV_WORDS (OV_COLS * 3 / 4)

// numpy's float -> uint8 cast on x86-64 goes through int32 (NaN / out of range -> INT_MIN) and
// keeps the low byte: 300 -> 44, -1 -> 255, 1e10 -> 0 (checked against numpy 2.2).
__device__ __forceinline__ uint8_t np_u8(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return 0;
    return (uint8_t)(uint32_t)(int32_t)v;
}

// sortable keys of doubles (monotone in the value for non-NaN inputs)
__device__ __forceinline__ uint64_t d2key(double d) {
    uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key2d(uint64_t k) {
    uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// ---- exportDICOM overlay ----------------------------------------------------------------------
__global__ void k_absmm_init(uint32_t *mm, int64_t nb) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nb) {
        mm[2 * v] = 0xffffffffu;
        mm[2 * v + 1] = 0u;
    }
}

// Per-volume min / max of |x| as float bits.  |NaN| sorts above +inf, so hi > 0x7f800000 flags a
// NaN (numpy's min and max then both return NaN).
__global__ __launch_bounds__(VH_TPB) void k_absminmax(const float *__restrict__ x, int64_t V,
                                                      uint32_t *__restrict__ mm) {
    const float *p = x + (int64_t)blockIdx.y * V;
    uint32_t lo = 0xffffffffu, hi = 0u;
    const int64_t stride = (int64_t)gridDim.x * VH_TPB;
    const int64_t t0 = (int64_t)blockIdx.x * VH_TPB + threadIdx.x;
    if ((V & 3) == 0) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p);
        const int64_t n4 = V >> 2;
        for (int64_t i = t0; i < n4; i += stride) {
            const float4 v = p4[i];
            const uint32_t a = __float_as_uint(v.x) & 0x7fffffffu, b = __float_as_uint(v.y) & 0x7fffffffu;
            const uint32_t c = __float_as_uint(v.z) & 0x7fffffffu, d = __float_as_uint(v.w) & 0x7fffffffu;
            lo = min(lo, min(min(a, b), min(c, d)));
            hi = max(hi, max(max(a, b), max(c, d)));
        }
    } else {
        for (int64_t i = t0; i < V; i += stride) {
            const uint32_t a = __float_as_uint(p[i]) & 0x7fffffffu;
            lo = min(lo, a);
            hi = max(hi, a);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
    __shared__ uint32_t s[2][VH_TPB / VH_WAVE];
    const int w = threadIdx.x / VH_WAVE;
    if ((threadIdx.x & (VH_WAVE - 1)) == 0) {
        s[0][w] = lo;
        s[1][w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < VH_TPB / VH_WAVE; ++k) {
            lo = min(lo, s[0][k]);
            hi = max(hi, s[1][k]);
        }
        atomicMin(&mm[2 * blockIdx.y], lo);
        atomicMax(&mm[2 * blockIdx.y + 1], hi);
    }
}

// One block = one row r, 64 columns, up to 64 slices of one volume.  Reads the block's
// contiguous [c][z] run of N4 / defect, composes the RGB triples into LDS in [z][c][3] order and
// writes each slice's 192-byte row segment out as dwords.
__global__ __launch_bounds__(VH_TPB) void k_overlay(const float *__restrict__ n4,
                                                    const uint8_t *__restrict__ def,
                                                    const uint32_t *__restrict__ mm, int64_t R,
                                                    int64_t C, int64_t Z, int ncc,
                                                    uint8_t *__restrict__ rgb) {
    __shared__ uint32_t sbuf[OV_ZC * OV_WORDS];
    uint8_t *sb = reinterpret_cast<uint8_t *>(sbuf);
    const int cchunk = blockIdx.x % ncc, zchunk = blockIdx.x / ncc;
    const int64_t r = blockIdx.y, vol = blockIdx.z;
    const int64_t c0 = (int64_t)cchunk * OV_COLS, z0 = (int64_t)zchunk * OV_ZC;
    const int nc = (int)min((int64_t)OV_COLS, C - c0), nz = (int)min((int64_t)OV_ZC, Z - z0);
    const uint32_t lo = mm[2 * vol], hi = mm[2 * vol + 1];
    const bool nan = hi > 0x7f800000u;
    const float mn = __uint_as_float(lo), mx = __uint_as_float(hi);
    const float rng = mx - mn;   // np.max(x) - np.min(x), float32
    const int64_t base = ((vol * R + r) * C + c0) * Z + z0;
    const int n = nc * nz;
    for (int j = threadIdx.x; j < n; j += VH_TPB) {
        const int c = j / nz, z = j - c * nz;
        const int64_t idx = base + (int64_t)c * Z + z;
        const float x = fabsf(n4[idx]);
        const uint8_t d = def[idx];
        uint8_t bw = 0;
        if (!nan) {
            const float v = (rng != 0.f) ? (x - mn) / rng : x;   // normalize (:233-237)
            bw = np_u8((double)(v * 255.f));                      // * (2**8 - 1), astype uint8
        }
        const uint8_t g = d == 0 ? bw : (uint8_t)0;
        const int o = (z * nc + c) * 3;
        sb[o] = (uint8_t)(g + (d == 1 ? 255 : 0));
        sb[o + 1] = g;
        sb[o + 2] = g;
    }
    __syncthreads();
    const int64_t plane = R * C * 3;
    const int64_t out0 = ((vol * Z + z0) * R + r) * C * 3 + c0 * 3;
    if ((C & 3) == 0 && nc == OV_COLS) {   // dword stores: each slice segment is 48 aligned words
        for (int w = threadIdx.x; w < nz * OV_WORDS; w += VH_TPB) {
            const int z = w / OV_WORDS, k = w - z * OV_WORDS;
            reinterpret_cast<uint32_t *>(rgb + out0 + z * plane)[k] = sbuf[w];
        }
    } else {
        const int seg = nc * 3;
        for (int bidx = threadIdx.x; bidx < nz * seg; bidx += VH_TPB) {
            const int z = bidx / seg, k = bidx - z * seg;
            rgb[out0 + z * plane + k] = sb[bidx];
        }
    }
}

void vh_overlay_launch(hipStream_t s, const float *d_n4, const uint8_t *d_def, int64_t R,
                       int64_t C, int64_t Z, int64_t nb, uint32_t *d_mm, uint8_t *d_rgb) {
    const int64_t V = R * C * Z;
    if (nb > 65535 || R > 65535) throw VhError{VH_ERR_ARG, "overlay: batch or rows out of range"};
    k_absmm_init<<<(unsigned)((nb + VH_TPB - 1) / VH_TPB), VH_TPB, 0, s>>>(d_mm, nb);
    VH_CHECK_LAUNCH();
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(1024, (V + VH_TPB * 16 - 1) / (VH_TPB * 16)));
    k_absminmax<<<dim3((unsigned)per, (unsigned)nb), VH_TPB, 0, s>>>(d_n4, V, d_mm);
    VH_CHECK_LAUNCH();
    const int ncc = (int)((C + OV_COLS - 1) / OV_COLS);
    const int nzc = (int)((Z + OV_ZC - 1) / OV_ZC);
    k_overlay<<<dim3((unsigned)(ncc * nzc), (unsigned)R, (unsigned)nb), VH_TPB, 0, s>>>(
        d_n4, d_def, d_mm, R, C, Z, ncc, d_rgb);
    VH_CHECK_LAUNCH();
}

// ---- screenShot montage -----------------------------------------------------------------------
struct MontageArgs {
    const void *proton;   // float32 or float64 volume
    const void *hp;
    const float *n4;
    const uint8_t *mborder;
    const uint8_t *def;
    const double *ci;     // nullable: blank CI panel (the reference's except: CI = blank, :478-479)
    const double *parula; // [prow][3]
    int64_t prow;
    int p64, h64;         // 1: float64 volume, 0: float32
    int64_t R, C, Z;
    int64_t r0, nr, c0, nc, s0, ns;
};

__device__ __forceinline__ double load_as_double(const void *p, int is64, int64_t i) {
    return is64 ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
}

// min / max over the crop of proton, HPvent and N4 (keys[2a] = min, keys[2a+1] = max)
__global__ __launch_bounds__(VH_TPB) void k_crop_minmax(MontageArgs a, uint64_t *keys) {
    const int64_t n = a.nr * a.nc * a.ns;
    uint64_t lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    for (int64_t t = (int64_t)blockIdx.x * VH_TPB + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * VH_TPB) {
        const int64_t s = t % a.ns, j = (t / a.ns) % a.nc, i = t / (a.ns * a.nc);
        const int64_t idx = ((a.r0 + i) * a.C + a.c0 + j) * a.Z + a.s0 + s;
        const uint64_t k0 = d2key(load_as_double(a.proton, a.p64, idx));
        const uint64_t k1 = d2key(load_as_double(a.hp, a.h64, idx));
        const uint64_t k2 = d2key((double)a.n4[idx]);
        lo[0] = min(lo[0], k0); hi[0] = max(hi[0], k0);
        lo[1] = min(lo[1], k1); hi[1] = max(hi[1], k1);
        lo[2] = min(lo[2], k2); hi[2] = max(hi[2], k2);
    }
    for (int q = 0; q < 3; ++q) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[q] = min(lo[q], (uint64_t)__shfl_xor((unsigned long long)lo[q], o));
            hi[q] = max(hi[q], (uint64_t)__shfl_xor((unsigned long long)hi[q], o));
        }
        if ((threadIdx.x & (VH_WAVE - 1)) == 0) {
            atomicMin((unsigned long long *)&keys[2 * q], (unsigned long long)lo[q]);
            atomicMax((unsigned long long *)&keys[2 * q + 1], (unsigned long long)hi[q]);
        }
    }
}

// the screenShot normalize (:460-464) in the array's own float type, widened to float64
__device__ __forceinline__ double norm_val(const void *p, int is64, int64_t idx, double mn,
                                           double mx) {
    if (is64) {
        const double x = static_cast<const double *>(p)[idx];
        const double rng = mx - mn;
        return rng == 0.0 ? x : (x - mn) / rng;
    }
    const float x = static_cast<const float *>(p)[idx];
    const float fmn = (float)mn, rng = (float)mx - (float)mn;
    return (double)(rng == 0.f ? x : (x - fmn) / rng);
}

// One thread per montage pixel.  Grid row g of the 7 x ns montage holds panel g, column s holds
// crop slice s (skimage.util.montage, grid_shape=(7, ns), padding 0: images fill row-major).
__global__ __launch_bounds__(VH_TPB) void k_montage(MontageArgs a, const uint64_t *keys,
                                                    uint8_t *__restrict__ img,
                                                    int32_t *__restrict__ err) {
    const int64_t W = a.ns * a.nc, H = 7 * a.nr;
    const int64_t t = (int64_t)blockIdx.x * VH_TPB + threadIdx.x;
    if (t >= W * H) return;
    const int64_t y = t / W, x = t - y * W;
    const int g = (int)(y / a.nr);
    const int64_t i = y - g * a.nr, s = x / a.nc, j = x - s * a.nc;
    const int64_t idx = ((a.r0 + i) * a.C + a.c0 + j) * a.Z + a.s0 + s;
    double rv = 0.0, gv = 0.0, bv = 0.0;
    if (g == 2 || g == 3) {
        const int q = g - 2;
        rv = gv = bv = norm_val(q == 0 ? a.proton : a.hp, q == 0 ? a.p64 : a.h64, idx,
                                key2d(keys[2 * q]), key2d(keys[2 * q + 1]));
    } else if (g >= 4) {
        const double n = norm_val(a.n4, 0, idx, key2d(keys[4]), key2d(keys[5]));
        if (g == 4) {          // N4*(~border) + {0,1,1}*border
            const bool bd = a.mborder[idx] != 0;
            rv = bd ? 0.0 : n;
            gv = bv = bd ? 1.0 : n;
        } else if (g == 5) {   // N4*(~defArr) + {defArr, 0, 0}
            const bool df = a.def[idx] != 0;
            rv = df ? 1.0 : n;
            gv = bv = df ? 0.0 : n;
        } else {               // N4*(CI==0) + parula[int(CI*64/40)]*(CI>0)
            const double ci = a.ci ? a.ci[idx] : 0.0;
            const double tt = ci * 64.0 / 40.0;
            if (tt != tt) {
                atomicOr(err, 2);   // int(NaN): ValueError
            } else if (!(tt < 9.2e18 && tt > -9.2e18) || (int64_t)tt >= a.prow ||
                       (int64_t)tt < -a.prow) {
                atomicOr(err, 1);   // parula index out of range: IndexError
            } else if (ci > 0.0) {
                const double *p = a.parula + 3 * (int64_t)tt;
                rv = p[0]; gv = p[1]; bv = p[2];
            } else if (ci == 0.0) {
                rv = gv = bv = n;
            }
        }
    }
    uint8_t *o = img + t * 3;
    o[0] = np_u8(rv * 255.0);
    o[1] = np_u8(gv * 255.0);
    o[2] = np_u8(bv * 255.0);
}

void vh_montage_run(hipStream_t s, int64_t R, int64_t C, int64_t Z, const void *proton, int p64,
                    const void *hp, int h64, const float *n4, const uint8_t *mborder,
                    const uint8_t *def, const double *ci, const double *parula, int64_t prow,
                    const int64_t crop[6], uint8_t *image) {
    MontageArgs a{};
    a.R = R; a.C = C; a.Z = Z;
    a.r0 = crop[0]; a.nr = crop[1]; a.c0 = crop[2]; a.nc = crop[3]; a.s0 = crop[4]; a.ns = crop[5];
    if (a.nr <= 0 || a.nc <= 0 || a.ns <= 0 || a.r0 < 0 || a.c0 < 0 || a.s0 < 0 ||
        a.r0 + a.nr > R || a.c0 + a.nc > C || a.s0 + a.ns > Z)
        throw VhError{VH_ERR_ARG, "montage: crop outside the volume"};
    if (prow <= 0) throw VhError{VH_ERR_ARG, "montage: empty colour table"};
    a.p64 = p64; a.h64 = h64; a.prow = prow;
    const size_t V = (size_t)(R * C * Z);
    std::vector<Buf<char>> owned;   // freed as the call ends, the stream drained on every path
    auto up = [&](const void *h, size_t bytes) -> void * {
        owned.emplace_back();
        owned.back().reserve(bytes);
        char *d = owned.back();
        if (h && bytes) HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
        return d;
    };
    int32_t herr = 0;
    uint64_t hkeys[6] = {~0ull, 0ull, ~0ull, 0ull, ~0ull, 0ull};
    const int64_t npix = 7 * a.nr * a.ns * a.nc;
    try {
        a.proton = up(proton, V * (p64 ? 8 : 4));
        a.hp = up(hp, V * (h64 ? 8 : 4));
        a.n4 = (const float *)up(n4, V * 4);
        a.mborder = (const uint8_t *)up(mborder, V);
        a.def = (const uint8_t *)up(def, V);
        a.ci = ci ? (const double *)up(ci, V * 8) : nullptr;
        a.parula = (const double *)up(parula, (size_t)prow * 3 * 8);
        uint64_t *d_keys = (uint64_t *)up(hkeys, sizeof(hkeys));
        int32_t *d_err = (int32_t *)up(&herr, sizeof(herr));
        uint8_t *d_img = (uint8_t *)up(nullptr, (size_t)npix * 3);
        const int64_t ncrop = a.nr * a.nc * a.ns;
        const int64_t mblocks = std::max<int64_t>(1, std::min<int64_t>(1024, (ncrop + VH_TPB - 1) / VH_TPB));
        k_crop_minmax<<<(unsigned)mblocks, VH_TPB, 0, s>>>(a, d_keys);
        VH_CHECK_LAUNCH();
        k_montage<<<(unsigned)((npix + VH_TPB - 1) / VH_TPB), VH_TPB, 0, s>>>(a, d_keys, d_img, d_err);
        VH_CHECK_LAUNCH();
        HIP_TRY(hipMemcpyAsync(image, d_img, (size_t)npix * 3, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&herr, d_err, sizeof(herr), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    if (herr & 2) throw VhError{VH_ERR_ARG, "cannot convert float NaN to integer (CI colour index)"};
    if (herr & 1) throw VhError{VH_ERR_INDEX, "CI colour index out of range of the colour table "
                                              "(int(CI*64/40), Vent_Analysis.py:482-484)"};
}

// ---- the montages of a device-resident batch (vh_batch_montage) -------------------------------
// Everything k_montage reads is resident after vh_batch_run: d_hp, n4_last(), d_mask, d_defect and
// (after vh_batch_ci) the int16 shell map with the table's radii.  Three kernels serve the whole
// batch: k_crop_layout (cropToData of every mask, from the run's mask statistics), k_crop_minmax_b
// (the crop minima / maxima of proton, HPvent and N4) and k_montage_b (all studies' pixels over their
// ragged crops, into one compact buffer).
#define MT_COLS VH_MT_COLS   // crop columns per workgroup
#define MT_ZC VH_MT_ZC       // crop slices per workgroup
#define MT_DRAWN 5     // panels 2..6 are composed; 0 and 1 are blank

// cropToData(mask, border=5) (Vent_Analysis.py:430-456) of every study, one workgroup each, from
// the flags and counts the run's mask pass left (mask != 0, which is what sum > 0 says of a uint8
// mask).  Index 0 never counts as non-empty (the reference multiplies the flags by the index list);
// rows and columns widen by 5 and clamp, slices do not.  A study with no counted row, column or
// slice -- the reference's IndexError -- gets zeros and status VH_ERR_EMPTY.  The column flags are
// derived from colcount: k_mask_finish may keep its own in LDS.
__global__ __launch_bounds__(VH_TPB) void k_crop_layout(const uint8_t *__restrict__ rowany,
                                                        const uint8_t *__restrict__ sliceany,
                                                        const int32_t *__restrict__ colcount,
                                                        int64_t R, int64_t C, int64_t Z,
                                                        int32_t *__restrict__ crop) {
    __shared__ int32_t s_lo[3], s_hi[3];
    const int64_t b = blockIdx.x, CZ = C * Z;
    if (threadIdx.x < 3) { s_lo[threadIdx.x] = INT_MAX; s_hi[threadIdx.x] = -1; }
    __syncthreads();
    int32_t lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    for (int64_t r = 1 + threadIdx.x; r < R; r += VH_TPB)
        if (rowany[b * R + r]) { lo[0] = min(lo[0], (int32_t)r); hi[0] = max(hi[0], (int32_t)r); }
    for (int64_t i = Z + threadIdx.x; i < CZ; i += VH_TPB)   // columns 1 .. C - 1
        if (colcount[b * CZ + i] > 0) {
            const int32_t c = (int32_t)((uint32_t)i / (uint32_t)Z);
            lo[1] = min(lo[1], c); hi[1] = max(hi[1], c);
        }
    for (int64_t z = 1 + threadIdx.x; z < Z; z += VH_TPB)
        if (sliceany[b * Z + z]) { lo[2] = min(lo[2], (int32_t)z); hi[2] = max(hi[2], (int32_t)z); }
    for (int q = 0; q < 3; ++q)
        if (hi[q] >= 0) { atomicMin(&s_lo[q], lo[q]); atomicMax(&s_hi[q], hi[q]); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *o = crop + b * 8;
        const bool ok = s_hi[0] >= 0 && s_hi[1] >= 0 && s_hi[2] >= 0;
        const int32_t r0 = max(s_lo[0] - 5, 0), r1 = min(s_hi[0] + 6, (int32_t)R);
        const int32_t c0 = max(s_lo[1] - 5, 0), c1 = min(s_hi[1] + 6, (int32_t)C);
        o[0] = ok ? r0 : 0; o[1] = ok ? r1 - r0 : 0;
        o[2] = ok ? c0 : 0; o[3] = ok ? c1 - c0 : 0;
        o[4] = ok ? s_lo[2] : 0; o[5] = ok ? s_hi[2] + 1 - s_lo[2] : 0;
        o[6] = ok ? VH_OK : VH_ERR_EMPTY;
        o[7] = 0;
    }
}

void vh_crop_layout_launch(vh_batch *b) {
    k_crop_layout<<<(unsigned)b->nb, VH_TPB, 0, b->stream>>>(b->d_rowany, b->d_sliceany, b->d_colcount,
                                                            b->R, b->C, b->Z, b->d_mt_crop);
    VH_CHECK_LAUNCH();
}

struct MtArgs {
    const MtStudy *st;
    int32_t nb;
    const float *proton;     // nullable: zeros (what the class substitutes for a missing proton)
    const float *hp, *n4;
    const uint8_t *mask, *def;
    const int16_t *shell;    // nullable: the blank CI panel
    const double *radii;
    int64_t nbs;
    double minvox;
    const double *parula;
    int64_t prow;
    int64_t R, C, Z, V;
    uint32_t *keys;          // [nb][6]
    int32_t *flag;           // [nb]
    uint8_t *img;
};

__global__ void k_mt_init(uint32_t *keys, int32_t *flag, int64_t nb) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nb) return;
    for (int q = 0; q < 3; ++q) { keys[6 * v + 2 * q] = 0xffffffffu; keys[6 * v + 2 * q + 1] = 0u; }
    flag[v] = 0;
}

// Crop minima / maxima of proton, HPvent and N4 of every study as sortable keys (order-free: integer
// atomics).  blockIdx.y = study; its crop rows are dealt to the blocks of the column, a row's
// [c][z] runs to the threads.
__global__ __launch_bounds__(VH_TPB) void k_crop_minmax_b(MtArgs a) {
    const int64_t b = blockIdx.y;
    const MtStudy s = a.st[b];
    if (s.nr == 0) return;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    const int n = s.nc * s.ns;   // < 2^31 (check_dims)
    for (int i = blockIdx.x; i < s.nr; i += gridDim.x) {
        const int64_t base = b * a.V + ((int64_t)(s.r0 + i) * a.C + s.c0) * a.Z + s.s0;
        for (int j = threadIdx.x; j < n; j += VH_TPB) {
            const int c = j / s.ns, z = j - c * s.ns;
            const int64_t idx = base + (int64_t)c * a.Z + z;
            const uint32_t k0 = f2key(a.proton ? a.proton[idx] : 0.f);
            const uint32_t k1 = f2key(a.hp[idx]), k2 = f2key(a.n4[idx]);
            lo[0] = min(lo[0], k0); hi[0] = max(hi[0], k0);
            lo[1] = min(lo[1], k1); hi[1] = max(hi[1], k1);
            lo[2] = min(lo[2], k2); hi[2] = max(hi[2], k2);
        }
    }
    __shared__ uint32_t s_k[6][VH_TPB / VH_WAVE];
    for (int q = 0; q < 3; ++q) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[q] = min(lo[q], (uint32_t)__shfl_xor((int)lo[q], o));
            hi[q] = max(hi[q], (uint32_t)__shfl_xor((int)hi[q], o));
        }
        if ((threadIdx.x & (VH_WAVE - 1)) == 0) {
            s_k[2 * q][threadIdx.x / VH_WAVE] = lo[q];
            s_k[2 * q + 1][threadIdx.x / VH_WAVE] = hi[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool mx = threadIdx.x & 1;
        uint32_t v = s_k[threadIdx.x][0];
        for (int w = 1; w < VH_TPB / VH_WAVE; ++w) v = mx ? max(v, s_k[threadIdx.x][w]) : min(v, s_k[threadIdx.x][w]);
        if (mx) atomicMax(&a.keys[6 * b + threadIdx.x], v);
        else atomicMin(&a.keys[6 * b + threadIdx.x], v);
    }
}

// screenShot's normalize (:460-464) of a float32 array, then uint8(. * 255) with the product in
// float64 (IMAGE is float64: the parula columns are)
__device__ __forceinline__ uint8_t mt_u8(float x, float mn, float rng) {
    const float v = rng != 0.f ? (x - mn) / rng : x;
    return np_u8((double)v * 255.0);
}

// t / d and the remainder for small non-negative t (< 2^16) and 1 <= d <= 256 with inv = 1.f / d: a
// float product and one correction step instead of an integer division per element
__device__ __forceinline__ int mt_divmod(int t, int d, float inv, int &rem) {
    int q = __float2int_rz(((float)t + 0.5f) * inv);
    rem = t - q * d;
    if (rem < 0) { --q; rem += d; }
    else if (rem >= d) { ++q; rem -= d; }
    return q;
}

// One workgroup = one crop row of one study, up to MT_COLS columns and MT_ZC slices of it.  It reads
// the contiguous [c][z] runs of that row once (proton, HPvent, N4, defect, the shell, and the mask's
// four neighbours for calculateBorder), composes the five drawn panels' RGB triples in LDS, one
// [c][3] row per panel and slice, and writes every row out: the image is [panel nr + i][s nc + j][3],
// so a row is a contiguous run of 3 ncw bytes (and consecutive slices follow each other when the
// crop is one chunk wide).  A run goes out as aligned dwords -- the LDS words shifted to the run's
// alignment -- with up to three head and tail bytes, whatever nc is; consecutive threads take
// consecutive dwords of consecutive runs.  The two blank panels are written as zeros by the same loop.
// LDS rows are padded to an odd number of words: the threads of a wave hold consecutive slices of a
// column, and 3 ncw bytes is a multiple of 32 words' worth of banks for a full chunk.
// The workgroup finds its study in the prefix MtStudy::wg0 (binary search; uniform, scalar loads).
#define MT_RSW_MAX ((MT_COLS * 3 / 4) | 1)
__global__ __launch_bounds__(VH_TPB) void k_montage_b(MtArgs a) {
    __shared__ uint32_t sbuf[MT_DRAWN * MT_ZC * MT_RSW_MAX];
    uint8_t *sb = reinterpret_cast<uint8_t *>(sbuf);
    const int64_t w = blockIdx.x;
    int b = 0, hi = a.nb;   // st[b].wg0 <= w < st[hi].wg0: the last such b is a study with workgroups
    while (hi - b > 1) {
        const int mid = (b + hi) >> 1;
        if (a.st[mid].wg0 <= w) b = mid; else hi = mid;
    }
    const MtStudy s = a.st[b];
    int64_t q = w - s.wg0;
    const int cchunk = (int)(q % s.ncc);
    q /= s.ncc;
    const int zchunk = (int)(q % s.nzc), i = (int)(q / s.nzc);
    const int j0 = cchunk * MT_COLS, z0 = zchunk * MT_ZC;
    const int ncw = min(MT_COLS, s.nc - j0), nz = min(MT_ZC, s.ns - z0);
    const int L = ncw * 3;                        // bytes of a row
    const int rsw = ((L + 3) >> 2) | 1;           // its LDS stride in words (odd), <= MT_RSW_MAX
    const int psz = MT_ZC * MT_RSW_MAX * 4;       // bytes of a panel in LDS
    // offsets inside a volume are < 2^31 (check_dims): 32-bit index arithmetic
    const int C = (int)a.C, Z = (int)a.Z;
    const int r = s.r0 + i, rm = max(r - 1, 0), rp = min(r + 1, (int)a.R - 1);
    const int64_t vb = (int64_t)b * a.V;
    const float *pr = a.proton ? a.proton + vb : nullptr, *hp = a.hp + vb, *n4 = a.n4 + vb;
    const uint8_t *m = a.mask + vb, *def = a.def + vb;
    const int16_t *shell = a.shell ? a.shell + vb : nullptr;
    const uint32_t *k = a.keys + 6 * b;
    const float mnP = key2f(k[0]), rgP = key2f(k[1]) - mnP;   // np.max(x) - np.min(x), float32
    const float mnH = key2f(k[2]), rgH = key2f(k[3]) - mnH;
    const float mnN = key2f(k[4]), rgN = key2f(k[5]) - mnN;
    const int n = ncw * nz;
    const float inz = 1.f / (float)nz;
    for (int j = threadIdx.x; j < n; j += VH_TPB) {
        int z;
        const int c = mt_divmod(j, nz, inz, z);
        const int cc = s.c0 + j0 + c, zz = s.s0 + z0 + z;
        const int cm = max(cc - 1, 0), cp = min(cc + 1, C - 1);
        const int idx = (r * C + cc) * Z + zz;
        const uint8_t p8 = mt_u8(pr ? pr[idx] : 0.f, mnP, rgP);
        const uint8_t h8 = mt_u8(hp[idx], mnH, rgH);
        const uint8_t n8 = mt_u8(n4[idx], mnN, rgN);
        // calculateBorder(mask) != 0: np.gradient along rows or columns, one-sided at the edges
        const bool bd = m[(rp * C + cc) * Z + zz] != m[(rm * C + cc) * Z + zz] ||
                        m[(r * C + cp) * Z + zz] != m[(r * C + cm) * Z + zz];
        const bool df = def[idx] != 0;
        uint8_t c0 = n8, c1 = n8, c2 = n8;   // the CI panel: N4 where CI == 0
        if (shell) {
            const int32_t sh = shell[idx];
            const double ci = sh >= 0 && sh < a.nbs ? a.radii[sh] * a.minvox : 0.0;   // k_ci_expand16's value
            const double tt = ci * 64.0 / 40.0;
            if (ci > 0.0) {
                if (!(tt < 9.2e18) || (int64_t)tt >= a.prow) {   // IndexError (:482-484)
                    atomicOr(&a.flag[b], 1);
                    c0 = c1 = c2 = 0;
                } else {
                    const double *pp = a.parula + 3 * (int64_t)tt;
                    c0 = np_u8(pp[0] * 255.0); c1 = np_u8(pp[1] * 255.0); c2 = np_u8(pp[2] * 255.0);
                }
            }
        }
        uint8_t *o = sb + z * rsw * 4 + c * 3;
        o[0] = p8; o[1] = p8; o[2] = p8;
        o += psz;
        o[0] = h8; o[1] = h8; o[2] = h8;
        o += psz;
        o[0] = bd ? (uint8_t)0 : n8;            // N4*(~border) + {0, 1, 1}*border
        o[1] = bd ? (uint8_t)255 : n8;
        o[2] = bd ? (uint8_t)255 : n8;
        o += psz;
        o[0] = df ? (uint8_t)255 : n8;          // N4*(~defArr) + {defArr, 0, 0}
        o[1] = df ? (uint8_t)0 : n8;
        o[2] = df ? (uint8_t)0 : n8;
        o += psz;
        o[0] = c0; o[1] = c1; o[2] = c2;
    }
    __syncthreads();
    // slot 0 of a run: its head and tail bytes; slots 1 ..: its aligned dwords
    const int slots = (L >> 2) + 2;
    const float islots = 1.f / (float)slots;
    const int64_t nc3 = (int64_t)s.nc * 3;
    const int64_t prow = (int64_t)s.nr * s.ns * nc3;                   // bytes of a panel
    uint8_t *img = a.img + s.off + ((int64_t)i * s.ns + z0) * nc3 + j0 * 3;   // off is 4-byte aligned (VH_MT_ALIGN)
    const int a0 = (int)((s.off + ((int64_t)i * s.ns + z0) * nc3 + j0 * 3) & 3);
    for (int g = 0; g < 7; ++g) {
        uint8_t *pg = img + g * prow;
        const int ag = (a0 + (int)((g * prow) & 3)) & 3;
        const int lp = g >= 2 ? (g - 2) * psz : 0;                     // the panel in LDS (read for g >= 2 only)
        const uint8_t *sp = sb + lp;
        for (int t = threadIdx.x; t < nz * slots; t += VH_TPB) {
            int d;
            const int zr = mt_divmod(t, slots, islots, d);
            const int64_t A = zr * nc3;                                // the run's start from pg
            const int h = min((4 - ((ag + (int)(A & 3)) & 3)) & 3, L); // head bytes up to the first aligned dword
            const int nd = (L - h) >> 2;                               // aligned dwords
            const int S = zr * rsw * 4;                                // the run in the panel's LDS
            if (d == 0) {
                const int tail = L - h - 4 * nd;                       // < 4
                for (int e = 0; e < h; ++e) pg[A + e] = g >= 2 ? sp[S + e] : (uint8_t)0;
                for (int e = L - tail; e < L; ++e) pg[A + e] = g >= 2 ? sp[S + e] : (uint8_t)0;
            } else if (d <= nd) {
                uint32_t v = 0u;
                if (g >= 2) {
                    const int bb = S + h + 4 * (d - 1), wi = (lp + bb) >> 2, sh = (bb & 3) * 8;
                    v = sbuf[wi];
                    if (sh) v = (v >> sh) | (sbuf[wi + 1] << (32 - sh));   // word wi + 1 starts inside the row
                }
                *reinterpret_cast<uint32_t *>(pg + A + h + 4 * (d - 1)) = v;
            }
        }
    }
}

void vh_montage_b_launch(vh_batch *b, bool proton, int64_t prow, bool ci_on) {
    hipStream_t st = b->stream;
    MtArgs a{};
    a.st = b->d_mt_st; a.nb = (int32_t)b->nb;
    a.proton = proton ? b->d_proton : nullptr;
    a.hp = b->d_hp; a.n4 = b->n4_last();
    a.mask = b->d_mask; a.def = b->d_defect;
    a.shell = ci_on ? b->d_ci_shell16 : nullptr;
    a.radii = b->d_ci_radii; a.nbs = b->state.ci_nbs(); a.minvox = b->state.ci_minvox();
    a.parula = b->d_mt_parula; a.prow = prow;
    a.R = b->R; a.C = b->C; a.Z = b->Z; a.V = b->V;
    a.keys = b->d_mt_keys; a.flag = b->d_mt_flag; a.img = b->d_mt_img;
    int64_t vox = 0;
    for (int64_t i = 0; i < b->nb; ++i) vox += (int64_t)b->mt_st[i].nr * b->mt_st[i].nc * b->mt_st[i].ns;
    const int64_t grid = b->mt_st[b->nb].wg0;
    // per crop voxel: the min/max pass (hp, N4, proton), then hp, N4, proton, defect, mask (its
    // neighbours come from the caches), the shell, and 21 bytes out
    const double per = (proton ? 12.0 : 8.0) * 2.0 + 2.0 + (ci_on ? 2.0 : 0.0) + 21.0;
    ScopedKTimer tm(b, "montage_b", per * (double)vox);
    k_mt_init<<<(unsigned)((b->nb + VH_TPB - 1) / VH_TPB), VH_TPB, 0, st>>>(a.keys, a.flag, b->nb);
    VH_CHECK_LAUNCH();
    if (grid == 0) return;   // every study empty
    const unsigned rows = (unsigned)std::min<int64_t>(b->R, 64);
    k_crop_minmax_b<<<dim3(rows, (unsigned)b->nb), VH_TPB, 0, st>>>(a);
    VH_CHECK_LAUNCH();
    k_montage_b<<<(unsigned)grid, VH_TPB, 0, st>>>(a);
    VH_CHECK_LAUNCH();
}
