// gs_blend_bwd.cuh -- the blend backward's two kernels (launchers: backward.hip): render_bwd_kernel, the select form
// (the default base backward), and render_bwd_rows_kernel<mode>, the rows form (the bwd_variant 0 fallback and the
// AMR, deterministic and aux backwards).  Both give one 16x16 tile to a single-wave workgroup, 4 pixels per lane
// (lane l: column l % 16 of the 4 row groups), and walk the tile's list back to front in LDS batches of 64 with the
// same load pipeline; what they really share is written once, everything else belongs to one kernel.
#pragma once

#include <type_traits>

#include "gs_blend.cuh"
#include "gs_device.cuh"
#include "gs_kernels.h"

namespace gsamd {

constexpr int kNG = 9;      // gradient terms per (pixel, Gaussian)
static_assert(kDetRow == kNG, "the deterministic backward's partial rows hold the nine terms");
constexpr int kAccRow = 9;   // LDS accumulator row (floats; odd stride: 9 scalar stores per row)
constexpr int kPPL = 4;      // pixels per lane: one wave64 covers the 16x16 tile (gs_blend.cuh mapping)
static_assert(kAuxDz == kAccRow && kAuxDz < kGradRow, "the aux backward's tenth sum takes a spare float of the row");
constexpr int kBwdBatch = 64;  // Gaussians per LDS batch

// The kernels' arguments (by value, as PreprocessArgs).  blend_bwd_params (backward.hip) fills all but the extras.
struct BlendBwdParams {
    int W, H;
    const uint32_t *ranges, *max_contrib, *point_list;
    const float2* means2D;
    const float4* conic_opacity;
    const float *colors, *final_Ts;
    const uint32_t* n_contrib;
    const float *dL_dpixels, *bg;
    float* grad_accum;  // (the deterministic backward: its partials array [R][kNG])
    int cull, gx;       // gx: tiles per row (AMR: 32-px tiles)
    const uint32_t *bucket_count, *bucket_list, *hdr;
    // extras of one rows mode each (null / 0 elsewhere)
    int amr_mode;                                 // kAmr
    const uint32_t* levels;                       // kAmr
    const float *depths, *dL_ddepth, *dL_dalpha;  // kAux (the two cotangents may be null)
};

// a . b over the three colour channels, as the explicit fma chain the compiler formed from a0 b0 + a1 b1 + a2 b2
// under contraction: left to contraction, which product of a sum of two is fused depends on the code around the
// expression, and the deterministic backward's bits would change with it.
__device__ __forceinline__ float fma_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return __builtin_fmaf(a2, b2, __builtin_fmaf(a0, b0, a1 * b1));
}

// The tile of block blockIdx.x: rank blockIdx.x of the heaviest-first order the forward render left in this image
// buffer's 256 work buckets.
__device__ __forceinline__ int bwd_block_tile(const uint32_t* __restrict__ bucket_count,
                                              const uint32_t* __restrict__ bucket_list, int lane) {
    int tile = (int)blockIdx.x;
    if (bucket_count) {
        // the bucket whose inclusive count first exceeds the rank (256 buckets: 4 per lane)
        const uint4 c4 = reinterpret_cast<const uint4*>(bucket_count)[lane];
        const uint32_t c = c4.x + c4.y + c4.z + c4.w;
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += y;
        }
        const uint32_t rank = blockIdx.x;
        const uint64_t past = __ballot(incl > rank);
        // counts that do not cover the grid exactly (an image buffer whose base forward render did not fill the
        // buckets, e.g. from another caller or size): every block takes the identity order instead, so each tile is
        // still processed exactly once
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total == gridDim.x && past != 0ull) {
            const int L = __builtin_ctzll(past);
            uint32_t r = rank - (uint32_t)__builtin_amdgcn_readlane((int)(incl - c), L);
            const uint32_t q0 = (uint32_t)__builtin_amdgcn_readlane((int)c4.x, L),
                           q1 = (uint32_t)__builtin_amdgcn_readlane((int)c4.y, L),
                           q2 = (uint32_t)__builtin_amdgcn_readlane((int)c4.z, L);
            int b = 4 * L;
            if (r >= q0) { r -= q0; b++;
                if (r >= q1) { r -= q1; b++;
                    if (r >= q2) { r -= q2; b++; } } }
            tile = (int)bucket_list[(size_t)b * gridDim.x + r];
        }
    }
    return tile;
}

// The lane's per-pixel state where the replay starts: T = T_final, last = n_contrib, dpx = dL_dpixel (zeros outside
// the image, and where the caller gave no colour cotangent: !have_dpix).  Returns the wave's max n_contrib -- entries
// at or past it are skipped by all its pixels -- and, per row group (the lane's k-th pixel), group_last[k] = the max
// n_contrib of its 64 pixels: entries at or past it are skipped by every pixel of the group.
__device__ __forceinline__ uint32_t load_pixel_state(const BlendBwdParams& p, const PixelSetT<kPPL>& px,
                                                     bool have_dpix, float (&T)[kPPL], uint32_t (&last)[kPPL],
                                                     float (&dpx)[kPPL][3], int (&group_last)[kPPL]) {
    const size_t plane = (size_t)p.H * p.W;
    uint32_t wave_last = 0;
#pragma unroll
    for (int k = 0; k < kPPL; k++) {
        const uint32_t pid = px.pid[k];
        T[k] = px.inside[k] ? p.final_Ts[pid] : 0.f;
        last[k] = px.inside[k] ? p.n_contrib[pid] : 0u;
        wave_last = max(wave_last, last[k]);
#pragma unroll
        for (int c = 0; c < 3; c++) dpx[k][c] = (px.inside[k] && have_dpix) ? p.dL_dpixels[c * plane + pid] : 0.f;
    }
    wave_last = wave_max_u32(wave_last);
#pragma unroll
    for (int k = 0; k < kPPL; k++) group_last[k] = __builtin_amdgcn_readfirstlane((int)wave_max_u32(last[k]));
    return wave_last;
}

// Software pipeline over the batches (vector-memory counters retire in issue order, so issue order decides what each
// wait covers): the next batch's point_list ids are loaded while this batch is blended (load_id), its Gaussian
// records are gathered (gather) before this batch's flush atomics are issued, so neither the id round trip nor the
// atomics' completion is waited for at the top of the next batch.
// (the hit codes ride with the records: loaded a batch ahead with them, so the batch's row masks wait for nothing the
// records did not -- loaded at the top of the batch, they cost one more memory round trip per batch, with the next
// batch's id load behind them in the same counter)
struct NextRecord {
    uint32_t id = 0, code = 0xfu;
    float2 xy = make_float2(0.f, 0.f);
    float4 co = make_float4(0.f, 0.f, 0.f, 0.f);
    float rgb[3] = {0.f, 0.f, 0.f};

    // entry e of the sorted list (codes: the forward's hit codes, or null)
    __device__ __forceinline__ void load_id(const BlendBwdParams& p, const uint8_t* codes, uint32_t e) {
        id = p.point_list[e];
        if (codes != nullptr) code = codes[e];
    }
    __device__ __forceinline__ void gather(const BlendBwdParams& p) {
        xy = p.means2D[id];
        co = p.conic_opacity[id];
        rgb[0] = p.colors[3 * id]; rgb[1] = p.colors[3 * id + 1]; rgb[2] = p.colors[3 * id + 2];
    }
    // Stage the record for the batch: (x, y, r, g) and the scaled conic / opacity as two b128 reads, b as one b32
    // (LDS cycles per wave-read: b128 4, b96 8, b64 / b32 2; b at a 16-B stride: one LDS address serves all three
    // record reads).  Returns the scaled record.
    __device__ __forceinline__ float4 stage(float4* s_a, float4* s_co, float4* s_b, int slot) const {
        float4 pc = splat_coef(co);
        // (+ 0: an add where the staged record takes the opacity, so the compiler forms the b128 store's register
        // tuple here, after the wait for the gather, instead of with a copy right behind the gather's issue at the
        // end of the previous batch -- which made every batch wait a full memory round trip there)
        pc.w = pc.w + 0.0f;
        s_a[slot] = make_float4(xy.x, xy.y, rgb[0], rgb[1]);
        s_co[slot] = pc;
        s_b[slot].x = rgb[2];
        return pc;
    }
    // Row mask of the record: the forward's exact hit code when it left them (gs_blend.cuh blend_tile_t: bit r = row
    // group r has a pixel that blended the entry, i.e. a pixel this backward takes it at), else the geometric cull.
    __device__ __forceinline__ uint32_t row_mask(bool use_codes, int cull, uint32_t ox, uint32_t oy,
                                                 uint32_t pstride) const {
        return use_codes ? code : cull ? splat_group_mask(xy, co, (float)ox, (float)oy, (float)pstride) : 0xfu;
    }
};

// The batch [top - cnt, top)'s slots each row group still has to visit: mk[k] = the published row masks cut to the
// slots j whose contributor top - 1 - j is below group_last[k] (and below the wave's max).  Returns their union.
__device__ __forceinline__ uint64_t batch_masks(const uint64_t* s_bal, int top, uint32_t wave_last,
                                                const int (&group_last)[kPPL], uint64_t (&mk)[kPPL]) {
    // first batch slot this wave needs: contributor = top-1-j < wave_last
    // (readfirstlane: wave_last is uniform after the xor-shuffle max, but the compiler cannot prove it; without this
    // the bit-scan loop of the caller is compiled as a divergent VALU loop)
    const int j0 = __builtin_amdgcn_readfirstlane(max(0, top - (int)wave_last));
    uint64_t todo = 0;
    const uint64_t lo_cut = j0 >= 64 ? 0ull : j0 > 0 ? ~0ull << j0 : ~0ull;
#pragma unroll
    for (int k = 0; k < kPPL; k++) {
        // slots j with contributor = top-1-j < group_last[k], i.e. j >= top - group_last[k]
        const int jk = top - group_last[k];
        const uint64_t gcut = jk <= 0 ? ~0ull : (jk >= 64 ? 0ull : ~0ull << jk);
        mk[k] = uniform_u64(s_bal[k]) & lo_cut & gcut;
        todo |= mk[k];
    }
    return todo;
}

// A Gaussian's sums (c0, c1, c2, s0 = sum t, sx = sum t dx, sy = sum t dy, sxx, sxy, syy) -> the reference's nine
// terms.  Output component fq (0..2 colours, 3 / 4 mean x / y, 5..7 conic, 8 opacity; 9, the aux dz, passes through)
// = ka * qa + kb * sy, where qa is the sum fq starts from (sx for 3 and 4) and pc the staged log2(e)-scaled record
// that gives o and the conic.
// kOT: the sums are of t' = o t (the select form's opacity-scaled runs): o leaves the mean / conic factors and
// divides the opacity sum.
template <bool kOT>
__device__ __forceinline__ float flush_term(int fq, float qa, float sy, float4 pc, float ddelx_dx, float ddely_dy) {
#pragma clang fp contract(fast)
    const float o = kOT ? 1.0f : pc.w;
    const float cx = pc.x * (-1.0f / kHalfLog2e), cy = pc.y * (-1.0f / kLog2e), cz = pc.z * (-1.0f / kHalfLog2e);
    const float ka = fq == 3 ? -o * cx * ddelx_dx
                   : fq == 4 ? -o * cy * ddely_dy
                   : (fq >= 5 && fq <= 7) ? -0.5f * o
                   : (kOT && fq == 8) ? 1.0f / pc.w : 1.0f;
    const float kb = fq == 3 ? -o * cy * ddelx_dx : fq == 4 ? -o * cz * ddely_dy : 0.0f;
    // (an explicit fma, as fma_dot3: the form the deterministic rows were built with)
    return __builtin_fmaf(ka, qa, kb * sy);
}

// The select form (the default, and the hottest kernel of a training step): a visit with SGPR-mask selects and
// per-batch compare sets, its two transposed sum registers parked in an LDS staging slot, and every 7 visits one
// 63-lane pass that sums the staged partials, forms the nine terms and adds them into grad_accum (the flush fused
// into the staging reduce). Runs of provably negative-definite entries with o <= 0.99 sum the opacity-scaled t'
// (backward.hip, the variants' history).
__global__ void __launch_bounds__(64, 4) render_bwd_kernel(BlendBwdParams p) {
#pragma clang fp contract(fast)
    constexpr int kB = kBwdBatch;
    __shared__ uint32_t s_id[2][kB];  // double-buffered: the next batch's ids land while this one flushes
    __shared__ float4 s_a[kB];        // the staged records (NextRecord::stage)
    __shared__ float4 s_co[kB];
    __shared__ float4 s_b[kB];
    __shared__ uint64_t s_bal[4];
    // The per-Gaussian sums are finished in groups of 7 Gaussians -- each visit parks its two transposed registers
    // (16 column partials of each of 8 values, swap_rows8_pk_t) in a staging slot, and one pass over 7 slots sums
    // them with 63 lanes at once (lane = 9 * slot + value) instead of 14 DPP adds per Gaussian.  Layout: reduce lane
    // l's 16 partials are 4 float4s at l * 4 + i * kStagePitch (i = 0..3), so each b128 read is 64 consecutive dwords
    // per 16 lanes; the pitch's 16-float pad spreads the writers' 4 column groups over all 64 banks.
    constexpr int kStageSlots = 7;
    constexpr int kStagePitch = 272;
    __shared__ __attribute__((aligned(16))) float s_stage[3 * kStagePitch + 256];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int tile = bwd_block_tile(p.bucket_count, p.bucket_list, lane);
    const uint32_t ox = (uint32_t)(tile % p.gx) * 16, oy = (uint32_t)(tile / p.gx) * 16;
    const uint2 range = reinterpret_cast<const uint2*>(p.ranges)[tile];
    const int n = (int)(range.y - range.x);
    int m = min(n, (int)p.max_contrib[tile]);
    if (m == 0) return;  // block-uniform

    const PixelSetT<kPPL> px = make_pixels_t<kPPL, 1>(p.W, p.H, ox, oy, 1);
    const float bg0 = p.bg[0], bg1 = p.bg[1], bg2 = p.bg[2];
    // row group k's pixel y is py0 + 4 k: exact small-integer floats, the same operand the forward subtracts (3 fewer
    // live registers than px.y[])
    const float py0 = px.y[0];
    // accum_rec . dL_dpix is all the reference's accum_rec / last_color recurrences (backward.cu:500-507) feed into
    // dL_dalpha, so each pixel carries that one scalar instead of 2 x 3.
    float T[kPPL], dpx[kPPL][3], acc_dot[kPPL];
    uint32_t last[kPPL];
    int group_last[kPPL];
    const uint32_t wave_last = load_pixel_state(p, px, true, T, last, dpx, group_last);
    // The background term folded into the recurrence -- with B = T_final bg.dL_dpix / T (so the reference's bg term
    // is -T_new B), acc_dot + B obeys the same accum recurrence as acc_dot and starts at bg.dL_dpix: dL_dalpha =
    // T_new (c.dL_dpix - (acc_dot + B)).
#pragma unroll
    for (int k = 0; k < kPPL; k++) acc_dot[k] = fma_dot3(bg0, bg1, bg2, dpx[k][0], dpx[k][1], dpx[k][2]);
    // The smallest n_contrib of each row group's image pixels (pixels outside the image count as started: their T and
    // dL/dpix are 0, so any finite alpha leaves their terms 0).  Entries with contributor below it are taken by every
    // pixel of the group: no per-pixel contributor test.
    uint32_t min_last = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kPPL; k++) min_last = min(min_last, wave_min_u32(px.inside[k] ? last[k] : 0xffffffffu));
    min_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)min_last);
    // (the wave max = max_contrib[tile] for a whole base tile)
    m = min(m, __builtin_amdgcn_readfirstlane((int)wave_last));
    if (m == 0) return;
    // (where the forward stored its hit codes: the header word, gs_layout.h hit_codes_of)
    const uint8_t* const codes = p.hdr != nullptr ? hit_codes_of(p.point_list, p.hdr[kHdrHitCodes]) : nullptr;
    const bool use_codes = codes != nullptr;
    const float ddelx_dx = (float)(0.5 * p.W);
    const float ddely_dy = (float)(0.5 * p.H);

    NextRecord nr;
    if (tid < min(kB, m)) {
        nr.load_id(p, codes, range.x + m - 1 - tid);
        nr.gather(p);
        s_id[0][tid] = nr.id;
    }
    // Staging reduce: lane (slot = lane / 9, value q = lane % 9) sums the 16 column partials of value q parked by
    // slot's Gaussian (za rows hold values swap_sum_slot(r), zb rows 4 + swap_sum_slot(r); swap_sum_slot is its own
    // inverse) and adds the reference's term into grad_accum.
    const int st_slot = lane / 9, st_q = lane - 9 * (lane / 9);
    for (int i = lane; i < 3 * kStagePitch + 256; i += 64) s_stage[i] = 0.f;
    // writer lane: row r = lane / 16 of za / zb holds values swap_sum_slot(r) / 4 + swap_sum_slot(r), column c = lane
    // % 16 is element c of that sum. zb's value v = 4 + swap_sum_slot(r) of (g4, s1, s2, g7) goes to output q = v
    // except s2 (v = 6) -> q = 8; g6 (q = 6) = dx x (g4's column partial), formed after the transposition by lanes
    // 0-15 (zb row 0 = g4), the other lanes' product into their dummy word: no ninth-value DPP tree.
    const int st_dst = ((lane & 15) >> 2) * kStagePitch + 4 * swap_sum_slot(lane >> 4) + (lane & 3);
    const int st_dst_b = [&] {
        const int v = 4 + swap_sum_slot(lane >> 4);
        return ((lane & 15) >> 2) * kStagePitch + 4 * (v == 6 ? 8 : v) + (lane & 3);
    }();
    // (the idle lanes 16-63 store into the 16-word pads of pitch rows 0-2, which the reduce never reads)
    const int st_g6 = lane < 16 ? ((lane & 15) >> 2) * kStagePitch + 4 * 6 + (lane & 3)
                                : ((lane - 16) >> 4) * kStagePitch + 256 + (lane & 15);
    int par = 0;
    for (int top = m; top > 0; top -= kB, par ^= 1) {  // entries [top-cnt, top), back to front
        const int cnt = min(kB, top);
        __syncthreads();
        uint32_t gm = 0;
        bool fastg = false;  // p2 <= 0 at every pixel of the tile, provably (below)
        if (tid < cnt) {
            const float4 pc = nr.stage(s_a, s_co, s_b, tid);
            // the reference's `power > 0` skip cannot fire (gs_blend.cuh)
            fastg = splat_form_safe(pc, fabsf(nr.xy.x - (float)ox), fabsf(nr.xy.y - (float)oy)) &&
                    (pc.w <= 0.99f && pc.w > 0.0f);
            gm = nr.row_mask(use_codes, p.cull, ox, oy, 1);
        }
        const int ntop = top - kB;  // the next batch: entries [ntop - ncnt, ntop)
        const bool has_next = ntop > 0 && tid < min(kB, ntop);
        publish_group_masks<1>(gm, s_bal);
        const uint64_t fast_mask = uniform_u64(__ballot(fastg));
        // (after the masks: nothing below waits on this load until the batch ends)
        if (has_next) nr.load_id(p, codes, range.x + ntop - 1 - tid);
        // every contributor of this batch (<= top - 1) below every row group's smallest n_contrib: all pixels take
        // its entries
        const bool bstarted = (uint32_t)(top - 1) < min_last;
        int nst = 0;      // staging slots in use (wave-uniform)
        uint64_t js = 0;  // batch slot j of staging slot s in bits [6 s, 6 s + 6)
        // The staging reduce finishes the reference's nine terms itself (lane 9 s + q holds accumulator entry q of
        // slot s's Gaussian; entries 4 and 5 -- sum t dx, sum t dy -- fetched by two lane shuffles) and adds them into
        // grad_accum: no accumulator rows in LDS, no per-batch flush pass, one atomic instruction per 7 Gaussians
        // kOT: runs of fast entries sum t' = alpha T dL_dalpha / G = o t (below): the flush takes o out of the mean /
        // conic factors and divides the opacity sum by it
        auto stage_reduce = [&](const int nslot, auto kOT) {
            constexpr bool kOT_ = decltype(kOT)::value;
            if (nslot == kStageSlots || lane < 9 * nslot) {
                const float* src = &s_stage[4 * lane];
                const float4 a = *reinterpret_cast<const float4*>(src);
                const float4 b = *reinterpret_cast<const float4*>(src + kStagePitch);
                const float4 c = *reinterpret_cast<const float4*>(src + 2 * kStagePitch);
                const float4 d = *reinterpret_cast<const float4*>(src + 3 * kStagePitch);
                const gs_f2 x0 = gs_f2{a.x, a.y} + gs_f2{b.x, b.y}, x1 = gs_f2{a.z, a.w} + gs_f2{b.z, b.w};
                const gs_f2 x2 = gs_f2{c.x, c.y} + gs_f2{d.x, d.y}, x3 = gs_f2{c.z, c.w} + gs_f2{d.z, d.w};
                const gs_f2 y = (x0 + x1) + (x2 + x3);
                const uint32_t jj = (uint32_t)(js >> (6 * st_slot)) & 63u;
                // lane 9 s + q: output component fq of q (entries 0..2 colours, 3 = sum t -> opacity (8), 4 = sum t
                // dx -> mean x (3), 5 = sum t dy -> mean y (4), 6..8 -> conic (5..7)); the flush's formula
                const float tot = y.x + y.y;
                const float g4 = __shfl(tot, 9 * st_slot + 4, 64), sy = __shfl(tot, 9 * st_slot + 5, 64);
                if (lane < 63) {
                    const int fq = st_q < 3 ? st_q : st_q == 3 ? 8 : st_q - 1;
                    const float qa = (fq == 3 || fq == 4) ? g4 : tot;
                    const float v = flush_term<kOT_>(fq, qa, sy, s_co[jj], ddelx_dx, ddely_dy);
                    if (v != 0.f) atomicAdd(&p.grad_accum[(size_t)s_id[par][jj] * kGradRow + fq], v);
                }
            }
        };
        __syncthreads();
        uint64_t mk[kPPL];
        uint64_t todo = batch_masks(s_bal, top, wave_last, group_last, mk);
        // One Gaussian (batch slot j, record staged in LDS) against the wave's pixels.  (Reading the next set bit's
        // record ahead, in two register sets used in turn, measured no faster: the 4 waves per SIMD already hide the
        // LDS latency.)
        auto visit = [&](const int j, const float2 xy, const float4 pc, const float4 cf, auto kFastT, auto kStartedT,
                         auto kSlotT) {
            constexpr bool kFast = decltype(kFastT)::value, kStarted = decltype(kStartedT)::value;
            constexpr int kSlot = decltype(kSlotT)::value;  // this entry's staging slot
            const uint32_t contributor = (uint32_t)(top - 1 - j);
            const float dx = xy.x - px.x;
            const float pa = (pc.x * dx) * dx, pb = pc.y * dx;  // the lane's pixels share x
            // Per pixel with t = G dL_dalpha the reference adds (backward.cu: 518-545) dL_dopacity += t; dL_dmean2D
            // += -o t (C d) * (W/2, H/2); dL_dconic += -o/2 t (dx^2, dx dy, dy^2).  A lane's pixels share dx, so it
            // sums s0 = sum t, s1 = sum t dy, s2 = sum t dy^2 and forms the six moments (s0, dx s0, s1, dx^2 s0, dx
            // s1, s2) once; the flush applies o, the conic and the constants.
            // (-0: x + -0 == x for every x, so the first visited row group's fma(a, b, -0) / -0 + t fold to a plain
            // v_mul / move instead of a 3-operand fma with an inline 0)
            float c0 = -0.f, c1 = -0.f, c2 = -0.f, s0 = -0.f, s1 = -0.f, s2 = -0.f;
            // The select form: a rejected pixel takes alpha = G = 0, i.e. rinv = 1 (T unchanged), dchannel = t = 0
            // and acc_dot += 0 -- the same bits as the predicate form for every accepted pixel, no exec-mask
            // bookkeeping: a visited Gaussian is always summed (with the forward's hit codes a visited row group has
            // a pixel that blended; under the geometric cull an all-rejected visit sums zeros, which the flush skips).
            // The selects take an SGPR-pair mask (gs_sel2_zero_v) and only the compares the entry needs: alpha >=
            // 1/255 always; contributor < n_contrib unless the batch is started for every pixel; power > 0 only for
            // Gaussians not provably negative definite (fast_mask).
#pragma unroll
            for (int k = 0; k < kPPL; k++) {
                if (!((mk[k] >> j) & 1ull)) continue;  // wave-uniform
                const float dy = xy.y - (py0 + (float)(4 * k));
                const float p2 = splat_p2(pa, pb, dy, pc);
                const float Gr = splat_exp(p2);
                const float ar = fminf(0.99f, pc.w * Gr);
                uint64_t msk = __builtin_amdgcn_fcmpf(ar, 1.0f / 255.0f, kFcmpUGE);
                if (!kFast || !kStarted) msk &= __builtin_amdgcn_uicmp(contributor, last[k], kIcmpULT);
                if (!kFast) msk &= __builtin_amdgcn_fcmpf(p2, 0.0f, kFcmpULE);
                // a fast entry (o <= 0.99, p2 <= 0: alpha = o G unclamped, bit for bit the rounded product): t' = o t
                // = alpha T (c - acc) = dchannel_dcolor diff -- no G select, one product fewer; the flush divides o
                // back out
                constexpr bool kOT = kFast;
                float G, alpha;
                if constexpr (kOT) alpha = gs_sel_zero_v(msk, ar);
                else gs_sel2_zero_v(msk, Gr, ar, G, alpha);
                const float rinv = __builtin_amdgcn_rcpf(1.f - alpha);
                T[k] = T[k] * rinv;
                const float dchannel_dcolor = alpha * T[k];
                // (c - accum_rec - B) . dL_dpix as one fma chain
                const float diff = __builtin_fmaf(cf.z, dpx[k][2],
                                                  __builtin_fmaf(cf.y, dpx[k][1],
                                                                 __builtin_fmaf(cf.x, dpx[k][0], -acc_dot[k])));
                acc_dot[k] = __builtin_fmaf(alpha, diff, acc_dot[k]);
                c0 = __builtin_fmaf(dchannel_dcolor, dpx[k][0], c0);
                c1 = __builtin_fmaf(dchannel_dcolor, dpx[k][1], c1);
                c2 = __builtin_fmaf(dchannel_dcolor, dpx[k][2], c2);
                const float t = kOT ? dchannel_dcolor * diff : G * (diff * T[k]);
                const float tdy = t * dy;
                s0 += t;
                s1 += tdy;
                s2 = __builtin_fmaf(tdy, dy, s2);
            }
            // s2 rides in the 8-value transposition (g6 = dx^2 s0 leaves it; g6's column partials are dx x g4's,
            // formed after it)
            float g[kNG] = {c0, c1, c2, s0, dx * s0, s1, s2, dx * s1, s2};
            float za, zb;
            swap_rows8_pk_t<false>(g, za, zb);
            const float w6 = dx * zb;
            s_stage[st_dst + 36 * kSlot] = za;
            s_stage[st_dst_b + 36 * kSlot] = zb;
            s_stage[st_g6 + (lane < 16 ? 36 * kSlot : 0)] = w6;
            js |= (uint64_t)j << (6 * kSlot);
        };
        using T1 = std::integral_constant<bool, true>;
        using T0 = std::integral_constant<bool, false>;
        // one copy of the loop per (all-safe, started) batch case, chosen once per batch -- per-entry branches
        // between the visit variants made the register allocator shuffle the loop-carried pixel state (8 v_mov per
        // entry) at every join.  Rounds of 7 entries, one unrolled copy of the visit per staging slot (slot offsets
        // as immediates, no per-entry slot counter or address VALU, the visited bit cleared by one s_andn2)
        auto run = [&](auto kFastT, auto kStartedT) {
            auto one = [&](auto kSlotT) {
                if (!todo) return;  // wave-uniform
                const int j = __builtin_ctzll(todo);
                todo &= ~(1ull << j);
                const float4 a4 = s_a[j];
                const float2 xy = make_float2(a4.x, a4.y);
                const float4 pc = s_co[j], cf = make_float4(a4.z, a4.w, s_b[j].x, 0.f);
                visit(j, xy, pc, cf, kFastT, kStartedT, kSlotT);
                nst = decltype(kSlotT)::value + 1;
            };
            while (todo) {
                one(std::integral_constant<int, 0>{});
                one(std::integral_constant<int, 1>{});
                one(std::integral_constant<int, 2>{});
                one(std::integral_constant<int, 3>{});
                one(std::integral_constant<int, 4>{});
                one(std::integral_constant<int, 5>{});
                one(std::integral_constant<int, 6>{});
                if (nst == kStageSlots) {
                    stage_reduce(kStageSlots, kFastT);
                    nst = 0;
                    js = 0ull;
                }
            }
            if (nst) stage_reduce(nst, kFastT);
            nst = 0;
        };
        // every entry this wave visits has a provably negative-definite form
        const bool bsafe = (todo & ~fast_mask) == 0ull;
        if (bsafe && bstarted) run(T1{}, T1{});
        else if (bsafe) run(T1{}, T0{});
        else run(T0{}, T0{});
        __syncthreads();
        if (has_next) {  // gathers for the next batch, ahead of the next round's flush atomics
            s_id[par ^ 1][tid] = nr.id;
            nr.gather(p);
        }
    }
}

// What the rows form is run for.  kAmr, kDet and kAux each extend the base; kAuxInv is kAux on 1 / z.
enum class BwdRows { kBase, kAmr, kDet, kAux, kAuxInv };

// The rows form: the predicate visit, full sums by transposition into LDS accumulator rows, one flush pass per batch
// -- one 64-B atomic row per (tile, Gaussian).
// kAmr (the foveated backward, an extension beyond parity; p.amr_mode != 0): block b = (32-px tile b / 4, sub-lattice
// (b & 1, (b >> 1) & 1)), its 16 x 16 pixels at stride 2 -- the pixels amr_render_kernel blended for that AMR round.
// amr_mode = k > 0: foveaStep k's image (round k of tiles with level >= k); < 0: render_once (rounds <= level).
// kDet (the deterministic backward): grad_accum is the caller's partials array [R][kNG] instead -- the flush stores
// the nine terms of sorted instance i (= range.x + its index in the tile's list) at row i with plain stores and
// issues no atomic; reduce_partials_kernel (backward.hip) sums each Gaussian's rows in a fixed order.  Every row
// below min(n, max_contrib[tile]) is written (zeros where the default flush adds nothing), the rows at or past it are
// never read.
// kAux (the depth / alpha maps' backward): depth and alpha are two more blend channels with features (z, 1),
// background (0, 0) and cotangents dL_ddepth / dL_dalpha (either may be null, as dL_dpixels then: zeros) replayed in
// the same walk -- dL/dalpha of every pair gains their terms, and a tenth per-Gaussian sum dL/dz = sum alpha T
// dL_ddepth goes to float kAuxDz of the Gaussian's grad_accum row (LDS rows of 10).
// kAuxInv (the inverse-depth / alpha maps' backward): kAux with the record's z replaced by f = 1 / z (inv_depth, the
// forward's quotient) -- features (f, 1), p.dL_ddepth the inverse-depth map's cotangent, and float kAuxDz takes
// dL/df = sum alpha T dL_dinvdepth.  (An instantiation of its own: kAux keeps its code, and the parameter block
// its layout.)
// (a template parameter: run-time branches cost the base kernel 12 %)
template <BwdRows kMode>
__global__ void __launch_bounds__(64, 4) render_bwd_rows_kernel(BlendBwdParams p) {
#pragma clang fp contract(fast)
    constexpr bool kAMR = kMode == BwdRows::kAmr, kDet = kMode == BwdRows::kDet;
    constexpr bool kInv = kMode == BwdRows::kAuxInv, kAux = kMode == BwdRows::kAux || kInv;
    constexpr int kRow = kAux ? kAccRow + 1 : kAccRow;  // LDS accumulator row of this mode
    constexpr int kB = kBwdBatch;
    __shared__ uint32_t s_id[2][kB];  // double-buffered: the next batch's ids land while this one flushes
    __shared__ float4 s_a[kB];        // the staged records (NextRecord::stage; kAux: z in s_b[].y)
    __shared__ float4 s_co[kB];
    __shared__ float4 s_b[kB];
    __shared__ float s_acc[kB * kRow];  // per-Gaussian sums, one row per batch slot, flushed per batch
    __shared__ uint64_t s_bal[4];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    int tile;
    uint32_t ox, oy;
    constexpr uint32_t pstride = kAMR ? 2 : 1;
    if constexpr (kAMR) {
        tile = (int)(blockIdx.x >> 2);
        const uint32_t sx = blockIdx.x & 1u, sy = (blockIdx.x >> 1) & 1u;
        const uint32_t round = sx == 0 ? (sy == 0 ? 1u : 4u) : (sy == 0 ? 3u : 2u);  // amr/cr/forward.cu:313-339
        const uint32_t L = min(p.levels[tile], 4u);
        if (p.amr_mode > 0 ? (round != (uint32_t)p.amr_mode || L < round) : round > L) return;
        ox = (uint32_t)(tile % p.gx) * 32 + sx;
        oy = (uint32_t)(tile / p.gx) * 32 + sy;
    } else {
        tile = bwd_block_tile(p.bucket_count, p.bucket_list, lane);
        ox = (uint32_t)(tile % p.gx) * 16;
        oy = (uint32_t)(tile / p.gx) * 16;
    }
    const uint2 range = reinterpret_cast<const uint2*>(p.ranges)[tile];
    const int n = (int)(range.y - range.x);
    int m = kAMR ? n : min(n, (int)p.max_contrib[tile]);
    if (m == 0) return;  // block-uniform

    const PixelSetT<kPPL> px = make_pixels_t<kPPL, 1>(p.W, p.H, ox, oy, pstride);
    const float bg0 = p.bg[0], bg1 = p.bg[1], bg2 = p.bg[2];
    const float py0 = px.y[0];  // (row group k's pixel y: py0 + 4 k stride, as render_bwd_kernel)
    float T[kPPL], nbg[kPPL], dpx[kPPL][3], acc_dot[kPPL];
    float dax[kAux ? kPPL : 1][2];  // kAux: (dL_ddepth, dL_dalpha) of the pixel
    uint32_t last[kPPL];
    int group_last[kPPL];
    const uint32_t wave_last = load_pixel_state(p, px, !kAux || p.dL_dpixels != nullptr, T, last, dpx, group_last);
#pragma unroll
    for (int k = 0; k < kPPL; k++) {
        if constexpr (kAux) {
            dax[k][0] = (px.inside[k] && p.dL_ddepth) ? p.dL_ddepth[px.pid[k]] : 0.f;
            dax[k][1] = (px.inside[k] && p.dL_dalpha) ? p.dL_dalpha[px.pid[k]] : 0.f;
        }
        // (-T_final / (1 - alpha)) * bg.dL_dpix = nbg * 1/(1 - alpha)
        nbg[k] = -T[k] * fma_dot3(bg0, bg1, bg2, dpx[k][0], dpx[k][1], dpx[k][2]);
        acc_dot[k] = 0.f;
    }
    // the wave max = max_contrib[tile] for a whole base tile; AMR: no per-tile max_contrib was recorded for the
    // sub-lattice, the wave max is the block's
    if constexpr (kDet) {
        // rows [wave max, min(n, max_contrib)) -- none when max_contrib is this forward's -- are read by the
        // reduction and visited by no batch: zeros
        const int mw = min(m, __builtin_amdgcn_readfirstlane((int)wave_last));
        float* part = p.grad_accum + (size_t)range.x * kNG;
        for (int i = mw * kNG + lane; i < m * kNG; i += 64) part[i] = 0.f;
    }
    m = min(m, __builtin_amdgcn_readfirstlane((int)wave_last));
    if (m == 0) return;
    // (where the forward stored its hit codes: the header word, gs_layout.h hit_codes_of)
    const uint8_t* const codes =
        (!kAMR && p.hdr != nullptr) ? hit_codes_of(p.point_list, p.hdr[kHdrHitCodes]) : nullptr;
    const bool use_codes = codes != nullptr;
    const float ddelx_dx = (float)(0.5 * p.W);
    const float ddely_dy = (float)(0.5 * p.H);
    const int comp = lane & 15;
    // flush: the accumulator-row entry each output component starts from
    const int ia = (kAux && comp == kAuxDz) ? kAuxDz : comp < 3 ? comp : comp == 8 ? 3 : comp < 5 ? 4 : comp + 1;

    NextRecord nr;
    float nz = 0.f;  // kAux: the Gaussian's view-space depth (kAuxInv: its inverse), carried with the record
    if (tid < min(kB, m)) {
        nr.load_id(p, codes, range.x + m - 1 - tid);
        nr.gather(p);
        if constexpr (kAux) nz = kInv ? inv_depth(p.depths[nr.id]) : p.depths[nr.id];
        s_id[0][tid] = nr.id;
    }
    int par = 0;
    for (int top = m; top > 0; top -= kB, par ^= 1) {  // entries [top-cnt, top), back to front
        const int cnt = min(kB, top);
        __syncthreads();
        uint32_t gm = 0;
        if (tid < cnt) {
            nr.stage(s_a, s_co, s_b, tid);
            if constexpr (kAux) s_b[tid].y = nz;
            gm = nr.row_mask(use_codes, p.cull, ox, oy, pstride);
        }
        const int ntop = top - kB;  // the next batch: entries [ntop - ncnt, ntop)
        const bool has_next = ntop > 0 && tid < min(kB, ntop);
        publish_group_masks<1>(gm, s_bal);
        // (after the masks: nothing below waits on this load until the batch ends)
        if (has_next) nr.load_id(p, codes, range.x + ntop - 1 - tid);
        uint64_t written = 0;  // batch slots whose sum rows were stored
        __syncthreads();
        uint64_t mk[kPPL];
        uint64_t todo = batch_masks(s_bal, top, wave_last, group_last, mk);
        while (todo) {
            // One Gaussian (batch slot j, record staged in LDS) against the wave's pixels.
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 a4 = s_a[j];
            const float2 xy = make_float2(a4.x, a4.y);
            const float4 pc = s_co[j], cf = make_float4(a4.z, a4.w, s_b[j].x, kAux ? s_b[j].y : 0.f);
            const uint32_t contributor = (uint32_t)(top - 1 - j);
            const float dx = xy.x - px.x;
            const float pa = (pc.x * dx) * dx, pb = pc.y * dx;  // the lane's pixels share x
            // (the lane's moments and their -0 seeds: as render_bwd_kernel's visit)
            float c0 = -0.f, c1 = -0.f, c2 = -0.f, s0 = -0.f, s1 = -0.f, s2 = -0.f;
            float c3 = 0.f;  // kAux: sum alpha T dL_ddepth (cf.w = z)
            bool any = false;
#pragma unroll
            for (int k = 0; k < kPPL; k++) {
                if (!((mk[k] >> j) & 1ull)) continue;  // wave-uniform: culled for this row group
                const float dy = xy.y - (py0 + (float)(4 * k * (int)pstride));
                const float p2 = splat_p2(pa, pb, dy, pc);  // the forward's bits
                const float G = splat_exp(p2);
                const float alpha = fminf(0.99f, pc.w * G);
                // The reference's three per-pixel `continue`s (backward.cu:466-482) as one predicate: only
                // wave-uniform branches save SIMD time, and nested ones make the compiler re-zero g[] on every skip
                // path.  (contributor >= last also covers pixels outside the image.)
                const bool ok = contributor < last[k] && !(p2 > 0.0f) && !(alpha < 1.0f / 255.0f);
                if (!ok) continue;
                any = true;
                const float rinv = __builtin_amdgcn_rcpf(1.f - alpha);
                T[k] = T[k] * rinv;
                const float dchannel_dcolor = alpha * T[k];
                // sum_ch (c - accum_rec) dL_dpix, with accum_rec . dL_dpix advanced by the reference's recurrence
                // (backward.cu:500-507)
                float c_dot = fma_dot3(cf.x, cf.y, cf.z, dpx[k][0], dpx[k][1], dpx[k][2]);
                if constexpr (kAux) {  // the channels (z, 1)
                    c_dot += cf.w * dax[k][0] + dax[k][1];
                    c3 = __builtin_fmaf(dchannel_dcolor, dax[k][0], c3);
                }
                // The reference advances accum_rec at the NEXT contributor from the stored (last_alpha, last_color);
                // advancing it here with the same operands gives the same bits and needs no per-pixel "last" state.
                const float diff = c_dot - acc_dot[k];
                // (an explicit fma, as fma_dot3)
                const float dL_dalpha = __builtin_fmaf(nbg[k], rinv, diff * T[k]);
                acc_dot[k] = __builtin_fmaf(alpha, diff, acc_dot[k]);
                c0 = __builtin_fmaf(dchannel_dcolor, dpx[k][0], c0);
                c1 = __builtin_fmaf(dchannel_dcolor, dpx[k][1], c1);
                c2 = __builtin_fmaf(dchannel_dcolor, dpx[k][2], c2);
                const float t = G * dL_dalpha;
                const float tdy = t * dy;
                s0 += t;
                s1 += tdy;
                s2 = __builtin_fmaf(tdy, dy, s2);
            }
            if (__ballot(any) == 0ull) continue;  // wave-uniform
            // full sums by transposition: 2 values per row leader + g8 in lane 63
            float g[kNG] = {c0, c1, c2, s0, dx * s0, s1, dx * (dx * s0), dx * s1, s2};
            float za, zb;
            swap_sum9(g, za, zb);
            if constexpr (kAux) {  // the tenth sum: the plain DPP tree, total in lane 63
                c3 = dpp_add<0x111, 0xf, true>(c3);   // row_shr:1
                c3 = dpp_add<0x112, 0xf, true>(c3);   // row_shr:2
                c3 = dpp_add<0x114, 0xf, true>(c3);   // row_shr:4
                c3 = dpp_add<0x118, 0xf, true>(c3);   // row_shr:8
                c3 = dpp_add<0x142, 0xa, false>(c3);  // row_bcast:15
                c3 = dpp_add<0x143, 0xc, false>(c3);  // row_bcast:31
            }
            if ((lane & 15) == 15) {
                float* row = &s_acc[j * kRow];
                const int q = swap_sum_slot(lane >> 4);
                row[q] = za;
                row[4 + q] = zb;
                if (lane == 63) {
                    row[8] = g[8];
                    if constexpr (kAux) row[kAuxDz] = c3;
                }
            }
            written |= 1ull << j;
        }
        __syncthreads();
        if (has_next) {  // gathers for the next batch, ahead of the flush atomics
            s_id[par ^ 1][tid] = nr.id;
            nr.gather(p);
            if constexpr (kAux) nz = kInv ? inv_depth(p.depths[nr.id]) : p.depths[nr.id];
        }
        // Flush: 16 lanes per Gaussian row, 4 rows per wave instruction (one 64-B memory-side atomic request per
        // (tile, Gaussian)).  (A full unroll lets the scheduler hoist all 64 LDS reads: 163 VGPRs.)
#pragma unroll 4
        for (int i = 0; i < kB / 4; i++) {
            const int r = (tid >> 4) + 4 * i;
            const bool wr = (written >> (r & 63)) & 1ull;
            if constexpr (kDet) {
                // a row no pixel took stores zeros: every row the reduction reads is written by this call
                if (r < cnt && comp < kNG && !wr)
                    p.grad_accum[(size_t)(range.x + (uint32_t)(top - 1 - r)) * kNG + comp] = 0.f;
            }
            if (r < cnt && comp < kRow && wr) {
                // v = ka * row[ia] + kb * row[5] (flush_term)
                const float* row0 = &s_acc[r * kRow];
                const float v = flush_term<false>(comp, row0[ia], row0[5], s_co[r], ddelx_dx, ddely_dy);
                if constexpr (kDet) p.grad_accum[(size_t)(range.x + (uint32_t)(top - 1 - r)) * kNG + comp] = v;
                else if (v != 0.f) atomicAdd(&p.grad_accum[(size_t)s_id[par][r] * kGradRow + comp], v);
            }
        }
    }
}

}  // namespace gsamd
