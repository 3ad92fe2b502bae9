// Split-K Winograd F(4x4, 3x3) kernel for a lone 32-channel output block (Cout == 32: the 64 -> 32 layers) on the fp32 matrix
// cores (v_mfma_f32_32x32x2_f32).  The F(4x4) scheme itself - transforms, filter image, region pairs, output stage - is described in
// wino4r_kernel.hip, whose conv_wino4r_kernel runs every other fp32 F(4x4) layer (and these, unsplit, under wino4_split = 0).
//
// Workgroup = 12 waves = 2 regions of 16x16 output pixels (32 Winograd tiles = the MFMA M dimension) x 32 output channels.
// Wave w = (input-channel half ch = w / 6, transform ROW xi = w % 6).  With 64-channel blocks ch is the output-channel half; for a
// lone 32-channel block the ch = 1 waves would multiply zero padding.  Instead both waves of a row work on the SAME 32 outputs and
// split the 8 input channels of a group: wave (ch, xi) runs only filter stage ch (channels 2 ch, 2 ch + 1 of both halo planes) of
// every group, from the ch = 0 slot of the unchanged filter image; the partial sums meet in the exchange image of the output stage
// (ch = 0 writes, ch = 1 adds).
//
// A wave reads the raw halo rows its row transform needs straight from LDS (8-byte reads: its two channels of every slot), forms
// t[j] = B^T[xi,:] d[:,j] and the six column points V[xi][0..5] in registers and multiplies them with U[xi][nu] on the MFMA
// (6 points x 16 accumulators = 96 registers); no transformed input ever touches LDS or HBM.
//
// Pipeline: the halo arrives 8 input channels at a time by LDS-DMA into a 3-deep ring, two groups ahead of its use (every wave
// issues two pieces per group, one at a time behind pinned MFMAs; nobody waits for a piece to land; ONE s_barrier per 8 channels).
// The filter fragments are private to a wave (nobody else reads them), so every wave streams its own 3-KB stage (6 points x 4 input
// channels x 32 output channels) by LDS-DMA into a private double buffer, ordered by its own counted vmcnt only - no barrier on the
// filter path.  All LDS-DMA goes through inline asm (wino4_consts.inc).  Per group a wave has two phases, T (row transform) and
// S (12 MFMAs); waves 4-11 run S one group late (phase rotation, see the K loop).
//
// LDS halo image (W4Lds::a_lane / a_row / a_col, wino4_lds_layout.h), 16-byte slots (4 channels): slot(g, y, x, h) = (g * 18 + P(y)) * 36 + h * 18 + P(x), where
// P(v) = {0, 5, 10, 14}[v % 4] + v / 4 regroups the 18 halo rows / columns by their phase modulo the tile stride 4.
// For a fixed tile offset (i, j) the 16 lanes of a ds_read group then read slots 36 * ty + tx + const:
// 36 = 4 (mod 16), so all 16 land on different 16-byte bank groups: conflict-free without padding.  The A-operand
// lane -> tile map follows the hardware's b128 lane groups (see tg / ty below).  (The row transform's 8-byte reads take half of every slot they touch:
// two-way on the banks under any placement of whole slots - tools/lds_bank_model.cpp, Site::floor.)
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "device_util.h"
#include "wino4_lds_layout.h"

namespace ecseg {

#include "wino4_consts.inc"
#define W4_HALO_RING 3
// raw image of this kernel: rows and columns regrouped by their phase modulo the tile stride (see the header), the two channel halves 18 slots apart
#define W4_HALO_SLOT(r, cc) const int h = (cc) >= 18 ? 1 : 0, hy = W4Lds::inv(r), hx = W4Lds::inv((cc) - h * 18)
#define W4_HALO_UPPER(cc) ((cc) >= 18)
#define W4_HALO_L W4Lds::Ring

// Row-transform pipeline depth (slots of in-flight halo reads beside the six direct ones; 0: rounds 1-3, column by column)
#ifndef ECSEG_W4_TSLOTS
#define ECSEG_W4_TSLOTS 4
#endif

// filter stages (wino4_filter_dma.inc): wt4[nb][stage][wave] is 768 floats, the wave's double buffer follows the ring
#define W4_FILTER_STRIDE (12 * 768 * 4)
#define W4_FILTER_LDS(buf) ((3 * W4_HS + W4Lds::bw_stage(wave, buf)) * 16u)

__global__ __launch_bounds__(768) void conv_wino4_kernel(ConvParams p, int regs_x, int regs_y, int npairs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* Hs = reinterpret_cast<f32x4*>(smem);              // [3][W4_HS]        halo ring (group g -> buffer g % 3)
    f32x4* Bs = Hs + 3 * W4_HS;                              // [12][2][W4_BWS]   per-wave filter stages

    const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;   // LDS byte address of the dynamic segment
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xi = wave % 6, ch = wave / 6;
    const int li = lane & 31, lh = lane >> 5;

#include "wino4_region.inc"
    // ---- filter DMA: wt4[nb][stage][wave][point pair nu / 2][lane = h * 32 + cout][nu % 2][k 2], 768 floats per wave and stage ----
    const unsigned long long w_base = (unsigned long long)(size_t)(p.wt + ((size_t)nb * nstages * 12 + xi) * 768);      // (both channel halves: the ch = 0 slot)
    f32x4* Bw = Bs + W4Lds::bw_stage(wave, 0);
#include "wino4_filter_dma.inc"

#include "wino4_lane_tile.inc"
    const int a_lane = W4Lds::a_lane(tg, ty, lh, tx);       // slot of halo pixel (4 ty, 4 tx) of the lane's tile

    // row transform of wave xi (row xi of B^T): t = c0 d[r0] + c1 d[r1] + c2 d[r2] + d[r3]  (rows 0 and 5: three terms)
    int rr0, rr1, rr2, rr3; float c0, c1, c2;
    switch (xi) {
        case 0:  rr0 = 0; rr1 = 2; rr2 = 4; rr3 = 4; c0 = KP;        c1 = KS;   c2 = 1.f; break;
        case 1:  rr0 = 1; rr1 = 2; rr2 = 3; rr3 = 4; c0 = -KA * KB2; c1 = -KB2; c2 = KA;  break;
        case 2:  rr0 = 1; rr1 = 2; rr2 = 3; rr3 = 4; c0 = KA * KB2;  c1 = -KB2; c2 = -KA; break;
        case 3:  rr0 = 1; rr1 = 2; rr2 = 3; rr3 = 4; c0 = -KA2 * KB; c1 = -KA2; c2 = KB;  break;
        case 4:  rr0 = 1; rr1 = 2; rr2 = 3; rr3 = 4; c0 = KA2 * KB;  c1 = -KA2; c2 = -KB; break;
        default: rr0 = 1; rr1 = 3; rr2 = 5; rr3 = 5; c0 = KP;        c1 = KS;   c2 = 1.f; break;
    }
    const int ro0 = W4Lds::a_row(rr0), ro1 = W4Lds::a_row(rr1), ro2 = W4Lds::a_row(rr2), ro3 = W4Lds::a_row(rr3);

    f32x16 acc[6];
#pragma unroll
    for (int v = 0; v < 6; ++v)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[v][e] = 0.f;

    f32x4 t[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) t[j] = f32x4{0.f, 0.f, 0.f, 0.f};    // (a wave writes only its own two components: keep the vectors defined)
    // ---- row transform of group grp: t[j] for the six halo columns of the lane's tile, the wave's two channels each ----
    // Rows 1-4 of B^T end in +1 (t = c0 d[r0] + c1 d[r1] + c2 d[r2] + d[r3]: three fmas), rows 0 and 5 have only three
    // terms, the last with +1 (t = c0 d[r0] + c1 d[r1] + d[r2]: three reads, two fmas) - for any point set of this shape.
    const bool inner_row = xi >= 1 && xi <= 4;
    auto transform = [&](int grp, auto c_src) __attribute__((always_inline)) {   // t[j][c_src + k] = row transform of channel c_src + k (k < 2, c_src = 2 ch) of the lane's slot
        constexpr int CS = decltype(c_src)::value, CN = 2;
        const f32x4* A = Hs + (grp % 3) * W4_HS + a_lane;
        constexpr int cp[6] = {W4Lds::a_col(0), W4Lds::a_col(1), W4Lds::a_col(2), W4Lds::a_col(3), W4Lds::a_col(4), W4Lds::a_col(5)};
        // scalar fmas on purpose (file is built with -fno-slp-vectorize): packed f32 VALU ops (v_pk_fma_f32) stall the
        // SIMD beside MFMAs, single v_fma_f32 hide in the matrix pipe's shadow
        // Software-pipelined (round 4): the phase used to be six LDS round trips behind each other (one per halo column:
        // 3 - 4 reads, wait, 12 fmas) and took 2200 - 3200 cycles per group - the three transforms of a SIMD's waves add up to the
        // group period (in-kernel stamps).  Now the LAST term of every column is read straight into t[j] (it enters the
        // chain with coefficient 1), the other reads go through NS rotating slots: each step waits for ONE read, accumulates it
        // into its column (two fmas) and re-issues the slot, so NS reads are always in flight.  The fma chain of a column runs in
        // the same order as before (innermost term first): results are bit-identical.
        constexpr int NS = ECSEG_W4_TSLOTS;
        // Only the wave's two channels CS, CS + 1 of every slot (round 4): 8-byte reads, half the fmas of a whole-slot transform - a
        // split wave multiplies half as often per group, so the row transform weighed twice as much per MFMA: 64 -> 32 channels ran
        // at 0.315 of the peak with whole slots, half the rate of the unsplit layers
        static_assert(CS == 0 || CS == 2, "one channel pair of the slot");
        auto rd = [&](int slot) __attribute__((always_inline)) -> f32x2 { return reinterpret_cast<const f32x2*>(A + slot)[CS / 2]; };
        f32x2 sl[NS];
        if (inner_row) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const f32x2 d = rd(ro3 + cp[j]);
#pragma unroll
                for (int c = 0; c < CN; ++c) t[j][CS + c] = d[c];
            }
#define W4_TRD(i) rd(((i) % 3 == 0 ? ro2 : (i) % 3 == 1 ? ro1 : ro0) + cp[(i) / 3])
#pragma unroll
            for (int k = 0; k < NS; ++k) sl[k] = W4_TRD(k);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                const float cf = i % 3 == 0 ? c2 : i % 3 == 1 ? c1 : c0;
#pragma unroll
                for (int c = 0; c < CN; ++c) t[i / 3][CS + c] = __builtin_fmaf(cf, sl[i % NS][c], t[i / 3][CS + c]);
                if (i + NS < 18) sl[i % NS] = W4_TRD(i + NS);
                __builtin_amdgcn_sched_barrier(0);
            }
#undef W4_TRD
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const f32x2 d = rd(ro2 + cp[j]);
#pragma unroll
                for (int c = 0; c < CN; ++c) t[j][CS + c] = d[c];
            }
#define W4_TRD(i) rd(((i) % 2 == 0 ? ro1 : ro0) + cp[(i) / 2])
#pragma unroll
            for (int k = 0; k < NS; ++k) sl[k] = W4_TRD(k);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const float cf = i % 2 == 0 ? c1 : c0;
#pragma unroll
                for (int c = 0; c < CN; ++c) t[i / 2][CS + c] = __builtin_fmaf(cf, sl[i % NS][c], t[i / 2][CS + c]);
                if (i + NS < 12) sl[i % NS] = W4_TRD(i + NS);
                __builtin_amdgcn_sched_barrier(0);
            }
#undef W4_TRD
        }
    };
#include "wino4_mfma_stage.inc"

    // Phase rotation.  Per 8-channel group a wave has two phases: T (halo LDS reads + row transform of its two channels,
    // latency-bound) and S (its one filter stage of the group: 12 MFMAs).  The barrier would keep the three waves of a SIMD
    // (w, w + 4, w + 8) in the same phase, with the matrix pipe idle while all of them transform.  So the barrier sits at a
    // different point of the phase sequence: waves 0-3 (one per SIMD) run T(g) S(g) after barrier g, waves 4-11 run S(g - 1) T(g):
    // while one class transforms, the other feeds the matrix pipe.  t[] lives in registers across the barrier; every wave executes
    // ngroups barriers and reads halo group g only between barriers g and g + 1.  The late waves' halo pieces of group g + 1 go
    // out in period g (inside S(g - 1)) and are waited for before barrier g + 1.  (Three classes with the stage cut into two
    // halves of 6 MFMAs: no gain, tools/experiments/wino4_split_three_classes.patch.)
// Priorities (round 4, A/B on one box): the MATRIX phases run above the transform (transform 0, matrix phases 1 / 2 by class): the
// transform is latency-bound on its LDS reads and loses nothing at priority 0, a ready MFMA no longer waits behind another wave's
// burst of transform fmas.  (Rounds 1-3: transform above the matrix phases; no priorities at all: -6 %.)
#define W4_PT 0
#define W4_PS(PR) ((PR) + 1)
// T(g) in the slot-pipelined form (the column-by-column two-channel transform of round 2 made the register allocator spill ~100
// registers).  S(g) = filter stage 2 g + CH of the image, private buffer g & 1: everything this wave issued has landed (vmcnt(0):
// the filter of this group and its halo pieces of group g + 1); streams the filter of group g + 1 and the halo of group g + 2
#define W4_TS(g, PR) do { __builtin_amdgcn_s_setprio(W4_PT); transform(g, std::integral_constant<int, 2 * CH>{}); \
                          __builtin_amdgcn_s_setprio(W4_PS(PR)); } while (0)
#define W4_SS(g) do { W4_SB(); W4_WAIT(0); W4_SB(); \
                      mfma_stage(CH, (g) & 1, ((g) + 1 < ngroups ? 2 * (g) + 2 : 2 * (g)) + CH, (g) + 2 < ngroups ? (g) + 2 : -1); } while (0)
    dma_halo_piece(0, std::integral_constant<int, 0>{});
    dma_halo_piece(0, std::integral_constant<int, 1>{});
    if (ngroups > 1) {
        dma_halo_piece(1, std::integral_constant<int, 0>{});
        dma_halo_piece(1, std::integral_constant<int, 1>{});
    }
    dma_filter_piece(ch, 0, std::integral_constant<int, 0>{});
    dma_filter_piece(ch, 0, std::integral_constant<int, 1>{});
    dma_filter_piece(ch, 0, std::integral_constant<int, 2>{});
    if (ngroups > 1) W4_WAIT(5); else W4_WAIT(3);            // halo group 0 has landed (group 1: before barrier 1, below)
    const int cls = wave >> 2;                               // waves 0-3: one per SIMD
    auto kloop = [&](auto chc) __attribute__((always_inline)) {          // (one copy of the loop per channel half: no branch inside)
        constexpr int CH = decltype(chc)::value;
        if (cls == 0) {
            for (int grp = 0; grp < ngroups; ++grp) {
                W4_BARRIER();
                W4_TS(grp, 0);
                W4_SS(grp);
            }
        } else {
            W4_BARRIER();
            W4_TS(0, 1);
            for (int grp = 1; grp < ngroups; ++grp) {
                W4_WAIT(0);
                W4_BARRIER();
                W4_SS(grp - 1);
                W4_TS(grp, 1);
            }
            W4_SS(ngroups - 1);
        }
    };
    if (ch == 0) kloop(std::integral_constant<int, 0>{}); else kloop(std::integral_constant<int, 1>{});
#undef W4_TS
#undef W4_SS

    // ---- output stage: one pass through a [xi][x][tile][32 couts] exchange image ----
    // wino4_combine.inc is written for the 64-channel kernels (two passes of 32 channels, an optional fused 1x1 head): this kernel
    // is its pass 0 without a head
    constexpr bool HEAD = false;
    constexpr int pass = 0;
#include "wino4_out_begin.inc"
    // fold the wave's own row (R = M[xi][:] A) into the exchange image; `add` (ch = 1): onto the partner's partial sums
    auto write_R = [&](auto add_c) __attribute__((always_inline)) {
        constexpr bool add = decltype(add_c)::value;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tl = (e & 3) + 8 * (e >> 2) + 4 * lh;               // accumulator row = tile slot
            const int fold_at = W4Lds::r_fold(xi, tl, li);
#include "wino4_fold.inc"
            if (add) {                                           // (this lane's four words: nobody else touches them in this phase)
                o[W4Lds::r_plane(0)] += r0; o[W4Lds::r_plane(1)] += r1; o[W4Lds::r_plane(2)] += r2; o[W4Lds::r_plane(3)] += r3;
            } else {
                o[W4Lds::r_plane(0)] = r0; o[W4Lds::r_plane(1)] = r1; o[W4Lds::r_plane(2)] = r2; o[W4Lds::r_plane(3)] = r3;
            }
        }
    };
    __syncthreads();                                         // main-loop LDS reads are done
    if (ch == 0) write_R(std::false_type{});
    __syncthreads();
    if (ch == 1) write_R(std::true_type{});
    __syncthreads();
#include "wino4_combine.inc"
}

// Eligibility beyond "3x3, stride 1, pad 1, same size" (checked by the caller): extents multiples of 16, input channels
// a multiple of 4 (>= 8), output channels a multiple of 32 (the filter image is zero padded to 8 / 64), 16-byte aligned views.
// The halo goes through a raw buffer descriptor with 32-bit lane offsets relative to the lower of a workgroup's two windows and
// 0x7fff0000 bytes of records: two neighbouring windows (whole launches) must fit that range - conv_wino4_span_ok(p, 2) - and so
// must the windows of one image that a region list can pair (cropped launches: conv_wino4_span_ok(p, per_image), checked by the
// caller before it hands over a list).  Beyond it the hardware would silently return zeros.
bool conv_wino4_span_ok(const ConvParams& p, int windows) {
    return (size_t)windows * p.in.h * p.in.w * (size_t)p.in.cs * 4 < 0x7fff0000ull;
}
bool conv_wino4_supported(const ConvParams& p) {
    return p.in.h == p.out.h && p.in.w == p.out.w && p.out.h % 16 == 0 && p.out.w % 16 == 0 && p.in.c % 4 == 0 &&
           p.in.c >= 8 && p.out.c % 32 == 0 && p.in.cs % 4 == 0 && p.out.cs % 4 == 0 && p.zero != nullptr && conv_wino4_span_ok(p, 2);
}

hipError_t launch_wino4_grid(const ConvParams& p, hipStream_t s, W4Kernel kern, DeviceOnce& attr_set, size_t kloop_lds, int nblocks) {
    const int regs_x = p.out.w / 16, regs_y = p.out.h / 16;
    const size_t nreg = p.lut != nullptr ? (size_t)(p.n / p.per_image) * p.lut_len : (size_t)p.n * regs_x * regs_y;
    const size_t npairs = (nreg + 1) / 2;
    const size_t grid = npairs * (size_t)nblocks;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull || !conv_wino4_span_ok(p, p.lut != nullptr ? p.per_image : 2)) return hipErrorInvalidValue;
    const size_t lds_epi = (size_t)W4Lds::EPI_FLOATS * 4;    // the output stage's exchange image lies over the K loop's buffers
    const size_t lds = lds_epi > kloop_lds ? lds_epi : kloop_lds;
    const hipError_t ea = attr_set.run([&] {                 // the attribute is per device
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(768), lds, s, p, regs_x, regs_y, (int)npairs);
    return hipGetLastError();
}

hipError_t launch_conv_wino4(const ConvParams& p, hipStream_t s) {
    if (p.out.c != 32 || p.head_w != nullptr) return hipErrorInvalidValue;    // (every other F(4x4) layer: launch_conv_wino4r / launch_conv_wino4s)
    static DeviceOnce attr_set;
    return launch_wino4_grid(p, s, conv_wino4_kernel, attr_set, (size_t)(3 * W4_HS + 12 * 2 * W4_BWS) * 16, 1);      // one output-channel block
}

}  // namespace ecseg
