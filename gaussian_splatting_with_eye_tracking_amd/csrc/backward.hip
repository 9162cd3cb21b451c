// backward.hip -- gradients on gfx950.
//
// render_bwd_kernel (gs_blend_bwd.cuh, launched here) follows base/cr/backward.cu:399-557 (renderCUDA
// backward): per pixel, back-to-front replay from n_contrib with the same
// T/accum_rec recurrences and the same nine per-(pixel, Gaussian) gradient
// terms.  What changes is where the sums go: the reference issues 9 global
// float atomics per contributing (pixel, Gaussian) pair -- on MI355X those
// are memory-side atomics at ~one 64-B request each, and 64 lanes hitting one
// address serialise.  Here one wave64 owns a whole 16x16 tile (4 pixels per
// lane, gs_blend.cuh) and, per Gaussian j of the LDS batch:
//   1. each lane sums its 4 pixels' terms as moments (the lane's pixels share
//      x), then the wave transposes the 64 lanes' values with permlane swaps
//      down to 16 column partials per value, parked in an LDS staging slot;
//   2. every 7 Gaussians, one 63-lane pass sums the staged partials (lane
//      9 s + q = value q of slot s), forms the reference's nine terms and adds
//      them into grad_accum[P][kGradRow] -- one atomic instruction per 7
//      (tile, Gaussian) pairs.
// (render_bwd_rows_kernel -- the fallback, AMR, deterministic and aux
// backwards -- sums by a full transposition into LDS rows and flushes one 64-B
// atomic row per (tile, Gaussian) at the end of each batch.)
// The backward also starts each tile at max(n_contrib) of its pixels
// (recorded by the forward) instead of the end of the range: entries past it
// are skipped by every pixel in the reference too.
//
// backward_gaussians_kernel fuses computeCov2DCUDA (base/cr/backward.cu:
// 144-274), preprocessCUDA (:346-396), computeColorFromSH (:20-139) and
// computeCov3D (:278-341) into one per-Gaussian pass that also emits the
// reference's dL_dmeans2D / dL_dconic / dL_dopacity / dL_dcolors layout from
// grad_accum, and writes every output element (zeros included).
#include <algorithm>

#include <hip/hip_ext.h>

#include "gs_blend.cuh"
#include "gs_blend_bwd.cuh"
#include "gs_bwd_math.cuh"
#include "gs_device.cuh"
#include "gs_kernels.h"

namespace gsamd {

// Backward variants (set_tuning("bwd_variant")).  Default: round 4's variant
// 11 -- the select form with SGPR-pair masks, per-batch compare sets, staged
// sums and the flush fused into the staging reduce: render_bwd 0.3707
// (variant 7) -> 0.3634 (masks) -> 0.3512 (s2 in the transposition) ->
// 0.3403 (unrolled slots) -> 0.3139 ms (fused flush) at config 2, 0.2887 ->
// 0.2433 at config 4 (profiles/r04b_ab_bwd*.log, r04e_ab_bwd*.log,
// r04l_ab_bwd*_m.log) -- plus, since round 5, the opacity-scaled sums
// (always on): in batches of provably negative-definite entries with o <= 0.99
// (alpha = o G unclamped, bit for bit the rounded product) the visit sums t'
// = alpha T (c - acc) . dL_dpix = o t, which needs no G select and one
// product less, and the flush takes o out of the mean / conic factors and
// divides the opacity sum by it (0.3116 -> 0.3063 ms at config 2, 0.2385 ->
// 0.2348 at config 4, profiles/r05d_ab_bwd_opt*.log).  Fallback (0): the
// predicate form with full sums in LDS rows (render_bwd_rows_kernel).
// Measured and removed (logs in profiles/): 2 waves x 2 px and 4 x 1
// geometries, half-wave DPP-tree sums, a 5-wave occupancy cap (spills), the
// un-fused staged forms, the heavy-tile split (r01h / DESIGN.md §8e), an
// XCD-compact tile order (r04u_ab_xcd*), plain-store / no-flush timing
// diagnostics.
constexpr int kDefaultBwdVariant = 2;
int g_bwd_variant = kDefaultBwdVariant;
void set_backward_variant(int v) { g_bwd_variant = v == 0 ? 0 : kDefaultBwdVariant; }

// The kernel arguments every blend backward launch shares (member order of BlendBwdParams; the extras zero).
// Tiles heaviest first: the forward render filled this image buffer's 256 work buckets (the kernels fall back to
// the identity order otherwise); the forward's hit codes are found through the header (gs_layout.h hit_codes_of).
static BlendBwdParams blend_bwd_params(int W, int H, const ImageView& img, const BinningView& b, const GeomView& g,
                                       const float* colors, const float* bg, const float* dL_dpix) {
    return BlendBwdParams{W, H, img.ranges, img.max_contrib, b.point_list, reinterpret_cast<const float2*>(g.means2D),
                          reinterpret_cast<const float4*>(g.conic_opacity), colors, img.accum_alpha, img.n_contrib,
                          dL_dpix, bg, g.grad_accum, g_cull, (W + 15) / 16, img.bucket_count, img.bucket_list, g.hdr};
}

void launch_render_backward(int W, int H, const ImageView& img, const BinningView& b, const GeomView& g,
                            const float* colors, const float* bg, const float* dL_dpix, hipStream_t s) {
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx == 0 || gy == 0) return;
    const BlendBwdParams p = blend_bwd_params(W, H, img, b, g, colors, bg, dL_dpix);
    // (the profiler's stage events, if any, ride on the dispatch itself)
    const DispatchEvents ev = take_dispatch_events();
    if (g_bwd_variant == 0)
        hipExtLaunchKernelGGL(render_bwd_rows_kernel<BwdRows::kBase>, dim3(gx * gy), dim3(64), 0, s, ev.start, ev.stop,
                              0, p);
    else
        hipExtLaunchKernelGGL(render_bwd_kernel, dim3(gx * gy), dim3(64), 0, s, ev.start, ev.stop, 0, p);
}

// The deterministic backward's second pass: grad_accum[p][0..8] of every
// visible Gaussian = the sum of its partial rows (render_bwd_rows_kernel kDet)
// over the tiles of its rectangle in ascending tile index, accumulated in
// float64 and rounded to float32 once, stored with a plain store -- the same
// bits whatever order the blend's workgroups ran in.
// It reads only what the backward is promised (point_list, the image and the
// geometry buffer): the Gaussian's row in a tile is found by binary search of
// the tile's list, which is sorted by (depth bits, Gaussian index) ascending
// -- the duplicate's key -- so the search is exact.  A rectangle whose area
// is not tiles_touched[p], or a tile whose list does not hold the Gaussian
// (buffers that are not one forward's), raises through the header word
// kHdrError and stores NaNs in the Gaussian's row: never a stale partial.
// Rows at or past min(n, max_contrib[tile]) are skipped, as the blend skips
// them.
// Work split: 16 lanes per Gaussian.  Each lane searches one tile of the
// rectangle (the ~log2 n dependent gathers of up to 16 tiles in flight at
// once), then lanes 0..8 read the found rows' nine values, one 36-B run per
// row, 16 rows' loads issued ahead of the float64 adds; rectangles of more
// than 16 tiles take further rounds.  (One thread per Gaussian was not built:
// it serialises the searches of a rectangle, reads each row as nine 4-B
// gathers at a 36-B stride, and a wave then lasts as long as its largest
// rectangle; most Gaussians touch 1-4 tiles, a few 80 and more.  One wave per
// Gaussian would idle 48+ lanes at the median.)
// Measured at config 2 (K = 4.44M instances, kernel trace,
// profiles/r07_deterministic_kernel_stats.csv): this kernel 0.734 ms, the
// kDet blend 0.411 ms (the default select-form blend 0.316 ms): the ~10 search
// steps of two dependent gathers each per instance are the cost, not the row
// reads.  Not built: the direct-slot layout (rows at a per-Gaussian offset +
// the tile's ordinal in the rectangle, no search) -- it needs an offset table,
// a zero-fill of the rows the blend's cut skips, and the rectangle in the
// blend's flush.
constexpr uint32_t kDetNone = 0xffffffffu;  // no row: the tile's entry is past the blend's cut, or the lane has no tile
__global__ void __launch_bounds__(256) reduce_partials_kernel(
    int P, uint32_t R, uint32_t gx, uint32_t gy, const int* __restrict__ radii, const float2* __restrict__ means2D,
    const float* __restrict__ depths, const uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ ranges,
    const uint32_t* __restrict__ max_contrib, const uint32_t* __restrict__ point_list,
    const float* __restrict__ partials, float* __restrict__ grad_accum, uint32_t* __restrict__ hdr,
    uint32_t err_token) {
    const int p = (int)((blockIdx.x * 256u + threadIdx.x) >> 4);
    const int sub = threadIdx.x & 15;
    if (p >= P) return;  // (whole 16-lane groups)
    const int rad = radii[p];
    if (rad <= 0) return;
    const float2 xy = means2D[p];
    const Rect r = get_rect(xy.x, xy.y, rad, 16, 16, gx, gy);
    const uint32_t w = r.x1 - r.x0;
    const uint32_t area = w * (r.y1 - r.y0);
    const uint64_t key = ((uint64_t)float_bits(depths[p]) << 32) | (uint32_t)p;
    bool bad = area != tiles_touched[p];
    double acc = 0.0;
    if (!bad) {
        for (uint32_t i0 = 0; i0 < area; i0 += 16) {  // row-major over the rectangle: ascending tile index
            uint32_t pos = kDetNone;
            const uint32_t i = i0 + (uint32_t)sub;
            if (i < area) {
                const uint32_t tile = (r.y0 + i / w) * gx + r.x0 + i % w;
                const uint2 range = reinterpret_cast<const uint2*>(ranges)[tile];
                const uint32_t end = min(range.y, R), beg = min(range.x, end);
                uint32_t lo = beg, hi = end;
                while (lo < hi) {  // lower bound of key in the tile's list
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    const uint32_t id = point_list[mid];
                    const uint64_t k = ((uint64_t)float_bits(depths[min(id, (uint32_t)(P - 1))]) << 32) | id;
                    if (k < key) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < end && point_list[lo] == (uint32_t)p) {
                    if (lo - beg < min(end - beg, max_contrib[tile])) pos = lo;
                } else {
                    bad = true;
                }
            }
            float v[16];
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const uint32_t q = (uint32_t)__shfl((int)pos, t, 16);
                v[t] = (q != kDetNone && sub < kNG) ? partials[(size_t)q * kNG + sub] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 16; t++) acc += (double)v[t];
        }
    }
    // the group's verdict: its 16 bits of the wave's ballot
    const uint64_t any_bad = __ballot(bad);
    const bool gbad = ((any_bad >> (threadIdx.x & 48u)) & 0xffffull) != 0ull;
    if (sub < kNG) grad_accum[(size_t)p * kGradRow + sub] = gbad ? __uint_as_float(0x7fc00000u) : (float)acc;
    if (gbad && sub == 0) hdr[kHdrError] = err_token;
}

void launch_render_backward_deterministic(int W, int H, int P, int R, const ImageView& img, const BinningView& b,
                                          const GeomView& g, const int* radii, const float* colors, const float* bg,
                                          const float* dL_dpix, float* partials, uint32_t err_token, hipStream_t s) {
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx == 0 || gy == 0 || P <= 0 || R <= 0) return;
    // the partials array in grad_accum's place (kDet); the forward's work
    // buckets still order the launch, heaviest tiles first
    BlendBwdParams p = blend_bwd_params(W, H, img, b, g, colors, bg, dL_dpix);
    p.grad_accum = partials;
    hipLaunchKernelGGL(render_bwd_rows_kernel<BwdRows::kDet>, dim3(gx * gy), dim3(64), 0, s, p);
    const unsigned groups = ((unsigned)P + 15u) / 16u;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(groups), dim3(256), 0, s, P, (uint32_t)R, (uint32_t)gx,
                       (uint32_t)gy, radii, reinterpret_cast<const float2*>(g.means2D), g.depths, g.tiles_touched,
                       img.ranges, img.max_contrib, b.point_list, partials, g.grad_accum, g.hdr, err_token);
}

// The blend backward with the depth and alpha maps' cotangents
// (gs_rasterizer_backward_aux): render_bwd_rows_kernel kAux, five channels in one
// walk of the tile lists, ten sums per Gaussian into g.grad_accum.
void launch_render_backward_aux(int W, int H, const ImageView& img, const BinningView& b, const GeomView& g,
                                const float* colors, const float* bg, const float* dL_dpix, const float* dL_ddepth,
                                const float* dL_dalpha, hipStream_t s, bool inverse) {
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx == 0 || gy == 0) return;
    const DispatchEvents ev = take_dispatch_events();
    BlendBwdParams p = blend_bwd_params(W, H, img, b, g, colors, bg, dL_dpix);
    p.depths = g.depths;
    p.dL_ddepth = dL_ddepth;
    p.dL_dalpha = dL_dalpha;
    if (inverse)
        hipExtLaunchKernelGGL(render_bwd_rows_kernel<BwdRows::kAuxInv>, dim3(gx * gy), dim3(64), 0, s, ev.start,
                              ev.stop, 0, p);
    else
        hipExtLaunchKernelGGL(render_bwd_rows_kernel<BwdRows::kAux>, dim3(gx * gy), dim3(64), 0, s, ev.start, ev.stop,
                              0, p);
}

// The depth map's direct term on the means: z = V[2] x + V[6] y + V[10] z +
// V[14] of the flat viewmatrix (transformPoint4x3), so dL_dmeans3D[i] +=
// dL/dz_i (V[2], V[6], V[10]) with dL/dz_i the row's float kAuxDz.  Runs
// after backward_gaussians_kernel, which wrote every dL_dmeans3D element.
// inv_depths (the inverse-depth map, null otherwise): the row's float is
// dL/df_i for f_i = 1 / z_i, and dL/dz_i = -f_i^2 dL/df_i with f_i the
// forward's quotient (inv_depth); nothing is divided for an invisible Gaussian.
__global__ void __launch_bounds__(256) aux_depth_to_means_kernel(int P, const int* __restrict__ radii,
                                                                 const float* __restrict__ grad_accum,
                                                                 const float* __restrict__ viewmatrix,
                                                                 float* __restrict__ dL_dmean3D,
                                                                 const float* __restrict__ inv_depths) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= P || radii[idx] <= 0) return;
    float dz = grad_accum[(size_t)idx * kGradRow + kAuxDz];
    if (inv_depths) {
        const float f = inv_depth(inv_depths[idx]);
        dz = -(f * f) * dz;
    }
    dL_dmean3D[3 * idx + 0] += dz * viewmatrix[2];
    dL_dmean3D[3 * idx + 1] += dz * viewmatrix[6];
    dL_dmean3D[3 * idx + 2] += dz * viewmatrix[10];
}

void launch_aux_depth_to_means(int P, const GeomView& g, const int* radii, const float* viewmatrix,
                               float* dL_dmean3D, hipStream_t s, bool inverse) {
    if (P <= 0) return;
    hipLaunchKernelGGL(aux_depth_to_means_kernel, dim3(((unsigned)P + 255u) / 256u), dim3(256), 0, s, P, radii,
                       g.grad_accum, viewmatrix, dL_dmean3D, inverse ? g.depths : nullptr);
}

// The foveated (AMR) blend backward: 32-px tile ranges, one wave per
// (tile, sub-lattice) block of 16 x 16 pixels at stride 2, only the blocks
// whose round the forward rendered (mode: foveaStep k > 0, or < 0 for
// render_once).  The 1 wave x 4 px geometry (gs_blend.cuh) only.
void launch_amr_render_backward(int W, int H, int mode, const ImageView& img, const BinningView& b,
                                const GeomView& g, const float* colors, const float* bg, const float* dL_dpix,
                                hipStream_t s) {
    const int tgx = (W + 31) / 32, tgy = (H + 31) / 32;
    if (tgx == 0 || tgy == 0 || mode == 0) return;
    BlendBwdParams p = blend_bwd_params(W, H, img, b, g, colors, bg, dL_dpix);
    p.amr_mode = mode;
    p.levels = img.levels;
    p.gx = tgx;
    hipLaunchKernelGGL(render_bwd_rows_kernel<BwdRows::kAmr>, dim3(4 * tgx * tgy), dim3(64), 0, s, p);
}

// (the per-Gaussian backward math: gs_bwd_math.cuh)

// kSH16: SH with M = 16 coefficients (degree-3 models): compile-time loops,
// 16-B loads and stores of the 192-B SH rows.
// small: when given, the 3-float outputs (dL_dmeans2D, dL_dmeans3D,
// dL_dscales, dL_dcolors at 0, 3, 6, 9) are returned there for the caller's
// coalesced stores instead of stored per thread at a 12-B stride.
// kDrgb: the host knows the forward stored d(rgb)/d(dir) (no SH coefficient
// path compiled: 114 instead of 164 VGPRs); the SH basis and dL/drgb are
// returned in sh19 (16 + 3) for the caller's staged dL_dsh stores.
// kAA: the backward of an antialiased forward (BackwardGaussArgs::antialiasing):
// acc[8] is dL/d(conic_opacity.w), conic_opacity.w = opacity * coef, so
// dL_dopacity = acc[8] * coef and acc[8] * opacity goes back through coef into
// the 2D covariance (gs_bwd_math.cuh cov2d_backward<true>): one more 4-B load
// per visible Gaussian.  Either form checks the header word the forward left
// (kHdrAntialias) against its own flag.
template <bool kHasSH, bool kHasScales, bool kSH16, bool kDrgb = false, bool kAA = false>
__device__ __forceinline__ void backward_gaussian_body(const BackwardGaussArgs& a,
                                                       const float* __restrict__ grad_accum,
                                                       const uint8_t* __restrict__ clamped_bits, int idx,
                                                       float* lrow, float (*small)[12] = nullptr,
                                                       float (*sh19)[19] = nullptr) {
    if (idx >= a.P) return;
    const bool vis = a.radii[idx] > 0;
    // Blend-stage gradients in the reference layout.
    float acc[kNG];
    if (vis) {
        const float4* row = reinterpret_cast<const float4*>(grad_accum + (size_t)idx * kGradRow);
        const float4 r0 = row[0], r1 = row[1];
        const float r2 = grad_accum[(size_t)idx * kGradRow + 8];
        acc[0] = r0.x; acc[1] = r0.y; acc[2] = r0.z; acc[3] = r0.w;
        acc[4] = r1.x; acc[5] = r1.y; acc[6] = r1.z; acc[7] = r1.w; acc[8] = r2;
    } else {
#pragma unroll
        for (int q = 0; q < kNG; q++) acc[q] = 0.f;
    }
    // a forward of the other mode wrote these buffers: raise through the header's
    // error word and poison the gradients rather than return wrong ones (uniform)
    if (a.err_word && (a.hdr[kHdrAntialias] != 0u) != kAA) {
        if (idx == 0) *a.err_word = a.err_token;
        if (vis) {
#pragma unroll
            for (int q = 0; q < kNG; q++) acc[q] = __uint_as_float(0x7fc00000u);
        }
    }
    // (dL_dcolor, dL_dconic, dL_dcov3D: NULL = not wanted -- the autograd
    // wrapper discards them unless the matching precomputed input was given;
    // the uniform tests cost nothing, the skipped stores 52 B per Gaussian)
    if (small) {
        (*small)[9] = acc[0];
        (*small)[10] = acc[1];
        (*small)[11] = acc[2];
        (*small)[0] = acc[3];
        (*small)[1] = acc[4];
        (*small)[2] = 0.f;
    } else {
        if (a.dL_dcolor) {
            a.dL_dcolor[3 * idx + 0] = acc[0];
            a.dL_dcolor[3 * idx + 1] = acc[1];
            a.dL_dcolor[3 * idx + 2] = acc[2];
        }
        a.dL_dmean2D[3 * idx + 0] = acc[3];
        a.dL_dmean2D[3 * idx + 1] = acc[4];
        a.dL_dmean2D[3 * idx + 2] = 0.f;
    }
    if (a.dL_dconic) reinterpret_cast<float4*>(a.dL_dconic)[idx] = make_float4(acc[5], acc[6], 0.f, acc[7]);
    // (kAA: acc[8] * coef, once cov2d_backward has the coefficient)
    if constexpr (!kAA) store_out1(&a.dL_dopacity[idx], acc[8], a.nt_out != 0);

    const int ncoef_out = a.M;  // dL_dsh is [P, M, 3]
    if (!vis) {
        if constexpr (kAA) store_out1(&a.dL_dopacity[idx], 0.f, a.nt_out != 0);
        if (small) {
#pragma unroll
            for (int i = 3; i < 9; i++) (*small)[i] = 0.f;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) a.dL_dmean3D[3 * idx + i] = 0.f;
        }
        if (a.dL_dcov3D) {
#pragma unroll
            for (int i = 0; i < 6; i++) a.dL_dcov3D[6 * idx + i] = 0.f;
        }
        if (kDrgb) {
#pragma unroll
            for (int i = 0; i < 19; i++) (*sh19)[i] = 0.f;
        } else if (kHasSH && kSH16) {
#pragma unroll
            for (int i = 0; i < 48; i++) lrow[i] = 0.f;
        } else if (kHasSH) {
            for (int i = 0; i < ncoef_out * 3; i++) a.dL_dsh[(size_t)idx * ncoef_out * 3 + i] = 0.f;
        }
        if (!small)
            for (int i = 0; i < 3; i++) a.dL_dscale[3 * idx + i] = 0.f;
        for (int i = 0; i < 4; i++) a.dL_drot[4 * idx + i] = 0.f;
        return;
    }

    // All loads up front (one memory round trip per thread).
    const float mx = a.means3D[3 * idx], my = a.means3D[3 * idx + 1], mz = a.means3D[3 * idx + 2];
    float cov3D[6];
    float4 qrot = make_float4(0.f, 0.f, 0.f, 0.f);
    float scl[3] = {0.f, 0.f, 0.f};
    if (kHasScales) {
        qrot = reinterpret_cast<const float4*>(a.rotations)[idx];
        scl[0] = a.scales[3 * idx + 0];
        scl[1] = a.scales[3 * idx + 1];
        scl[2] = a.scales[3 * idx + 2];
    }
    if (kHasScales && !a.has_cov_precomp) {
        // the forward's cov3D recomputed from the scale / rotation this pass
        // reads anyway (same code, no contraction: the same bits) instead of
        // 24 more bytes per Gaussian from the geometry buffer
        compute_cov3d(scl, qrot, a.scale_modifier, cov3D);
    } else {
        // cov3D_precomp given (alone, or together with scales / rotations: the
        // forward rendered the precomputed covariance, backward.cu:160 reads
        // it, and the scales still receive the cov3D backward, :395-396)
#pragma unroll
        for (int i = 0; i < 6; i++) cov3D[i] = a.cov3D[6 * idx + i];
    }
    float opac = 0.f;  // (kAA) the forward's input opacity
    if constexpr (kAA) opac = a.opacities[idx];
    float s[16][3];
    uint8_t cb = 0;
    // the forward's d(rgb)/d(dir) when it stored them: no SH coefficients read
    // (the header word is checked in the drgb-known kernel too: the host picks
    // that kernel from a registry keyed by the rows' address, which cannot see
    // a geometry buffer no forward of this library wrote)
    const bool use_drgb = kHasSH && a.drgb && a.hdr[kHdrDrgb] == 1u;  // uniform
    float d9[9];
    if (kHasSH) {
        if (use_drgb) {
            const float4* row = reinterpret_cast<const float4*>(a.drgb) + 3 * (size_t)idx;
            const float4 r0 = row[0], r1 = row[1], r2 = row[2];
            d9[0] = r0.x; d9[1] = r0.y; d9[2] = r0.z; d9[3] = r0.w;
            d9[4] = r1.x; d9[5] = r1.y; d9[6] = r1.z; d9[7] = r1.w; d9[8] = r2.x;
        } else if constexpr (!kDrgb) {
            load_sh_rows<kSH16>(a, idx, s, lrow);
        } else {
            // drgb-known kernel, rows not written: the preprocess's derivatives
            // from the coefficients (same operands as sh_backward_terms: the
            // same bits), in a phase of their own before the body's peak
            float c[16][3];
            load_sh_rows<true>(a, idx, c);
            const float dox = mx - a.campos[0], doy = my - a.campos[1], doz = mz - a.campos[2];
            const float len = sqrtf(dot3(dox, doy, doz, dox, doy, doz));
            float dx3[3], dy3[3], dz3[3];
            sh_ddir(a.D, c, dox / len, doy / len, doz / len, dx3, dy3, dz3);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                d9[k] = dx3[k];
                d9[3 + k] = dy3[k];
                d9[6 + k] = dz3[k];
            }
        }
        cb = clamped_bits[idx];
    }
    const Mat4 V = load_mat4(a.viewmatrix);
    const Mat4 Pm = load_mat4(a.projmatrix);

    // ---- computeCov2DCUDA (backward.cu:144-274)
    float dmean[3];
    float dcov[6];
    if constexpr (kAA) {
        float coef;
        cov2d_backward<true>(mx, my, mz, cov3D, acc[5], acc[6], acc[7], V, a.focal_x, a.focal_y, a.tan_fovx,
                             a.tan_fovy, dmean, dcov, acc[8] * opac, &coef);
        store_out1(&a.dL_dopacity[idx], acc[8] * coef, a.nt_out != 0);
    } else {
        cov2d_backward(mx, my, mz, cov3D, acc[5], acc[6], acc[7], V, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy,
                       dmean, dcov);
    }
    if (a.dL_dcov3D) {
#pragma unroll
        for (int i = 0; i < 6; i++) a.dL_dcov3D[6 * idx + i] = dcov[i];
    }

    // ---- preprocessCUDA backward (backward.cu:370-387): projection part (+=)
    proj_backward(mx, my, mz, Pm, acc[3], acc[4], dmean);

    // ---- computeColorFromSH backward (backward.cu:20-139)
    // (two calls with a constant pointer each: a run-time select of d9 or
    // nullptr made the compiler keep d9 in scratch memory)
    if constexpr (kDrgb) {
        float dsh_c[16], dRGB[3];
        sh_backward_terms(a.D, a.campos, mx, my, mz, s, cb, acc, dsh_c, dRGB, dmean, d9);
#pragma unroll
        for (int k = 0; k < 16; k++) (*sh19)[k] = dsh_c[k];
#pragma unroll
        for (int c = 0; c < 3; c++) (*sh19)[16 + c] = dRGB[c];
    } else if (kHasSH) {
        if (use_drgb) sh_backward<kSH16>(a, idx, mx, my, mz, s, cb, acc, dmean, kSH16 ? lrow : nullptr, d9);
        else sh_backward<kSH16>(a, idx, mx, my, mz, s, cb, acc, dmean, kSH16 ? lrow : nullptr, nullptr);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (small) (*small)[3 + i] = dmean[i];
        else a.dL_dmean3D[3 * idx + i] = dmean[i];
    }

    // ---- computeCov3D backward (backward.cu:278-341)
    if (kHasScales) {
        float dscale[3];
        float4 dq;
        cov3d_backward(qrot, scl, a.scale_modifier, dcov, dscale, dq);
        store_out4(reinterpret_cast<float4*>(a.dL_drot) + idx, dq, a.nt_out != 0);
        if (small) {
            (*small)[6] = dscale[0];
            (*small)[7] = dscale[1];
            (*small)[8] = dscale[2];
        } else {
            a.dL_dscale[3 * idx + 0] = dscale[0];
            a.dL_dscale[3 * idx + 1] = dscale[1];
            a.dL_dscale[3 * idx + 2] = dscale[2];
        }
    } else {
        if (small) {
            (*small)[6] = (*small)[7] = (*small)[8] = 0.f;
        } else {
            for (int i = 0; i < 3; i++) a.dL_dscale[3 * idx + i] = 0.f;
        }
        for (int i = 0; i < 4; i++) a.dL_drot[4 * idx + i] = 0.f;
    }
}

constexpr int kBgStageNt = 16;  // backward_gaussians_kernel stage flag: dL_dsh rows non-temporal


template <bool kHasSH, bool kHasScales, bool kSH16, bool kSmall = false, bool kAA = false>
__global__ void __launch_bounds__(256) backward_gaussians_kernel(BackwardGaussArgs a, const float* __restrict__ grad_accum,
                                                                 const uint8_t* __restrict__ clamped_bits, int stage) {
    constexpr bool kStage = kHasSH && kSH16;
    static_assert(!kSmall || kStage, "the small outputs are staged in the SH rows' LDS");
    __shared__ float s_dsh[kStage ? 256 * kShRow : 1];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    // (not needed when the forward stored d(rgb)/d(dir): the SH coefficients
    // are then never read)
    if (kStage && !(a.drgb && a.hdr[kHdrDrgb] == 1u)) {  // the workgroup's 256 SH rows in, wave-contiguous
        const int g0 = blockIdx.x * blockDim.x;
        const int n = min(256, a.P - g0);
        const float4* in = reinterpret_cast<const float4*>(a.shs) + (size_t)g0 * 12;
        if (n == 256) {
            // a full workgroup: the 12 loads of each thread issued back to back
            // (one memory round trip; the loop below waits for each load before
            // its LDS write -- 12 round trips at 3 waves per SIMD)
            float4 v[12];
#pragma unroll
            for (int k = 0; k < 12; k++) v[k] = in[threadIdx.x + 256 * k];
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const int f = threadIdx.x + 256 * k;
                float* r = s_dsh + (f / 12) * kShRow + 4 * (f % 12);
                r[0] = v[k].x; r[1] = v[k].y; r[2] = v[k].z; r[3] = v[k].w;
            }
        } else {
            for (int f = threadIdx.x; f < n * 12; f += 256) {
                const float4 v = in[f];
                float* r = s_dsh + (f / 12) * kShRow + 4 * (f % 12);
                r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
            }
        }
        __syncthreads();
    }
    // stage_small: the 3-float outputs too go out as the workgroup's
    // contiguous 3 x 256 floats per array (stores at a 12-B stride write one
    // 32-B granule per lane per instruction: ~+23 % write bytes at config 4,
    // profiles/r04d_cfg4_pmc_summary.json)
    float small[12];
    backward_gaussian_body<kHasSH, kHasScales, kSH16, false, kAA>(a, grad_accum, clamped_bits, idx,
                                                                  kStage ? s_dsh + threadIdx.x * kShRow : nullptr,
                                                                  kSmall ? &small : nullptr);
    if constexpr (kStage) {
        __syncthreads();
        const int g0 = blockIdx.x * blockDim.x;
        const int n = min(256, a.P - g0);
        float4* out = reinterpret_cast<float4*>(a.dL_dsh) + (size_t)g0 * 12;
        const bool nt = (stage & kBgStageNt) != 0;
        for (int f = threadIdx.x; f < n * 12; f += 256) {
            const float* r = s_dsh + (f / 12) * kShRow + 4 * (f % 12);
            store_out4(&out[f], make_float4(r[0], r[1], r[2], r[3]), nt);
        }
        if constexpr (kSmall) {
            __syncthreads();  // the SH rows are out: the LDS holds the small arrays now
            if (idx < a.P) {
#pragma unroll
                for (int i = 0; i < 12; i++) s_dsh[(i / 3) * 768 + 3 * threadIdx.x + i % 3] = small[i];
            }
            __syncthreads();
            const int nf = 3 * n;
            for (int f = threadIdx.x; f < 4 * 192; f += 256) {
                const int q = f / 192, i = f - 192 * q;
                float* d = q == 0 ? a.dL_dmean2D : q == 1 ? a.dL_dmean3D : q == 2 ? a.dL_dscale : a.dL_dcolor;
                if (!d || 4 * i >= nf) continue;
                const float* r = s_dsh + q * 768 + 4 * i;
                float* o = d + 3 * (size_t)g0 + 4 * i;
                if (4 * i + 4 <= nf) {
                    store_out4(reinterpret_cast<float4*>(o), make_float4(r[0], r[1], r[2], r[3]), a.nt_out != 0);
                } else {
                    for (int e = 0; e < 4 && 4 * i + e < nf; e++) o[e] = r[e];
                }
            }
        }
    }
}

// The drgb-known form (the training path: the forward stored d(rgb)/d(dir)):
// no SH-coefficient path (114 VGPRs: 4 waves per SIMD instead of 3) and the
// 192-B dL_dsh rows staged through a half-size LDS area in two rounds of 128
// Gaussians (25 KB, recomputed from the 16 basis values and dL/drgb each
// thread keeps), then the small outputs as in backward_gaussians_kernel.
template <bool kAA = false>
__global__ void __launch_bounds__(256) backward_gaussians_drgb_kernel(BackwardGaussArgs a,
                                                                      const float* __restrict__ grad_accum,
                                                                      const uint8_t* __restrict__ clamped_bits,
                                                                      int nt) {
    __shared__ float s_half[128 * kShRow];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    float small[12], sh19[19];
    backward_gaussian_body<true, true, true, true, kAA>(a, grad_accum, clamped_bits, idx, nullptr, &small, &sh19);
    const int g0 = blockIdx.x * blockDim.x;
    const int n = min(256, a.P - g0);
    const int ncoef = min((a.D + 1) * (a.D + 1), a.M);
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const int gh = g0 + 128 * h, nh = min(128, n - 128 * h);
        if (nh <= 0) break;  // block-uniform
        if (h) __syncthreads();  // the previous round's stores have read the area
        if ((int)(threadIdx.x >> 7) == h && idx < a.P) {
            float* r = s_half + (threadIdx.x & 127) * kShRow;
#pragma unroll
            for (int k = 0; k < 16; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) r[3 * k + c] = k < ncoef ? sh19[k] * sh19[16 + c] : 0.f;
        }
        __syncthreads();
        float4* out = reinterpret_cast<float4*>(a.dL_dsh) + (size_t)gh * 12;
        for (int f = threadIdx.x; f < nh * 12; f += 256) {
            const float* r = s_half + (f / 12) * kShRow + 4 * (f % 12);
            store_out4(&out[f], make_float4(r[0], r[1], r[2], r[3]), nt != 0);
        }
    }
    __syncthreads();  // the SH rows are out: the area holds the small arrays now
    if (idx < a.P) {
#pragma unroll
        for (int i = 0; i < 12; i++) s_half[(i / 3) * 768 + 3 * threadIdx.x + i % 3] = small[i];
    }
    __syncthreads();
    const int nf = 3 * n;
    for (int f = threadIdx.x; f < 4 * 192; f += 256) {
        const int q = f / 192, i = f - 192 * q;
        float* d = q == 0 ? a.dL_dmean2D : q == 1 ? a.dL_dmean3D : q == 2 ? a.dL_dscale : a.dL_dcolor;
        if (!d || 4 * i >= nf) continue;
        const float* r = s_half + q * 768 + 4 * i;
        float* o = d + 3 * (size_t)g0 + 4 * i;
        if (4 * i + 4 <= nf) {
            store_out4(reinterpret_cast<float4*>(o), make_float4(r[0], r[1], r[2], r[3]), a.nt_out != 0);
        } else {
            for (int e = 0; e < 4 && 4 * i + e < nf; e++) o[e] = r[e];
        }
    }
}

// The SH16 + scales kernel: the SH staging loads issued back to back and the
// 3-float outputs stored coalesced through LDS (stage_small: 0.0848 -> 0.0828
// ms at config 2, 0.529 -> 0.479 at config 4, profiles/r04j_ab_bg*.log); the
// drgb-known kernel when the host knows the forward stored d(rgb)/d(dir),
// below 4M Gaussians (config 2 0.0825 -> 0.0747 ms; at config 4 0.465 ->
// 0.486: 4 waves per SIMD help the latency-bound small scene, the two staging
// rounds cost the HBM-bound large one, profiles/r04n_ab_bg*.log, again with
// 48-B rows: 0.4617 vs 0.4703, r04y_ab_bg4.log).  The dL_dsh rows are stored
// with the non-temporal hint (0.0727 -> 0.0697 ms at config 2, 0.4582 ->
// 0.4393 at config 4, profiles/r04z4_ab_nt*.log); the other outputs and the
// input loads are not (+3 % / +9 %, r04z5_*, r04z7_*).  Measured and removed:
// the SH backward as its own kernel, per-thread SH staging loads, one-round
// drgb staging (r04z1_ab_bg*_stage4.log).
void launch_backward_gaussians(const BackwardGaussArgs& args, const GeomView& g, hipStream_t s) {
    if (args.P == 0) return;
    BackwardGaussArgs a = args;
    const dim3 grid((a.P + 255) / 256);
    const bool sh = a.shs != nullptr;
    const bool sh16 = sh && a.M == 16;
    const bool sc = a.scales != nullptr;
    a.nt_out = 0;
    // (each form twice: the antialiased one reads a.opacities)
    const bool aa = a.antialiasing != 0;
#define GS_BG_LAUNCH(A, B, C)                                                                                      \
    do {                                                                                                           \
        if (aa)                                                                                                    \
            hipLaunchKernelGGL((backward_gaussians_kernel<A, B, C, false, true>), grid, dim3(256), 0, s, a,        \
                               g.grad_accum, g.clamped, 0);                                                        \
        else                                                                                                       \
            hipLaunchKernelGGL((backward_gaussians_kernel<A, B, C>), grid, dim3(256), 0, s, a, g.grad_accum,       \
                               g.clamped, 0);                                                                      \
    } while (0)
    if (sh16 && sc && a.drgb && a.drgb_known && a.P < 4000000) {
        if (aa)
            hipLaunchKernelGGL(backward_gaussians_drgb_kernel<true>, grid, dim3(256), 0, s, a, g.grad_accum,
                               g.clamped, 1);
        else
            hipLaunchKernelGGL(backward_gaussians_drgb_kernel<false>, grid, dim3(256), 0, s, a, g.grad_accum,
                               g.clamped, 1);
    } else if (sh16 && sc) {
        if (aa)
            hipLaunchKernelGGL((backward_gaussians_kernel<true, true, true, true, true>), grid, dim3(256), 0, s, a,
                               g.grad_accum, g.clamped, kBgStageNt);
        else
            hipLaunchKernelGGL((backward_gaussians_kernel<true, true, true, true>), grid, dim3(256), 0, s, a,
                               g.grad_accum, g.clamped, kBgStageNt);
    } else if (sh16) GS_BG_LAUNCH(true, false, true);
    else if (sh && sc) GS_BG_LAUNCH(true, true, false);
    else if (sh) GS_BG_LAUNCH(true, false, false);
    else if (sc) GS_BG_LAUNCH(false, true, false);
    else GS_BG_LAUNCH(false, false, false);
#undef GS_BG_LAUNCH
}

}  // namespace gsamd

