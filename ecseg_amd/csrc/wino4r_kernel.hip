// Winograd F(4x4, 3x3) convolution on the fp32 matrix cores (gfx950): 36 instead of 144 multiplies per 4x4 output
// block, i.e. 4x fewer MFMAs than the direct convolution and 1.78x fewer than F(2x2,3x3), still exact-f32 fma chains
// (v_mfma_f32_32x32x2_f32).
//
//   Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A        d: 6x6 input tile, g: 3x3 filter, Y: 4x4 outputs
//
// The filter transform U = G g G^T is done once at model load (float64 on the host, filter_layout.hip: winograd4_filter).
//
// Workgroup = 12 waves = 2 regions of 16x16 output pixels (32 Winograd tiles = the MFMA M dimension) x 64 output
// channels.  Wave w = (channel half ch = w / 6, transform ROW xi = w % 6).  Per 8-channel group all 768 threads turn the raw
// halo into a t image in LDS ONCE per workgroup (row_pass: 576 half items, 24 fmas each; t[j] = B^T[xi,:] d[:,j]); a wave reads
// the six 16-byte columns of ITS row, forms the six column points V[xi][0..5] in registers and multiplies them with U[xi][nu]
// on the MFMA (6 points x 16 accumulators = 96 registers); no transformed input ever touches HBM.  After the K loop every
// wave folds its own row (R = M[xi][:] A) in registers, the six rows meet through LDS, and Y = A^T R + bias, activation is
// written as 16-byte stores (128-B segments per pixel).
//
// Pipeline: the raw halo arrives 8 input channels at a time by LDS-DMA into a double buffer, two groups ahead of its use; two
// barriers per group, the three waves of a SIMD rotated against them (see the K loop; the loop structure is conv_wino4s_kernel's,
// wino4s_kernel.hip).  The filter fragments are private to a wave (nobody else reads them), so every wave streams its own 3-KB
// stage (6 points x 4 input channels x 32 output channels) by LDS-DMA into a private double buffer, ordered by its own counted
// vmcnt only - no barrier on the filter path.  All LDS-DMA goes through inline asm (wino4_consts.inc).
//
// The output stage can also write the 2x2 max-pool of its result, finish a 1x1 head (<= 4 classes) and take its region
// list from a look-up table (demand-driven cropping) - see ConvParams in common.h.
//
// Where every value sits in LDS - raw image, t image, filter stages, exchange image - is decided in wino4_lds_layout.h (W4Lds): the kernel calls its
// functions and holds no address arithmetic of its own; tools/lds_bank_model.cpp walks the same functions against the LDS bank rule (round 9).
//
// History (round 6): until then every wave read the raw halo rows of its transform row straight from LDS and ran
// the row transform itself (24 raw slots + 72 fmas per group instead of six columns); this kernel replaced that one with
// bit-identical results, 1 - 6 % faster per layer.  The per-wave scheme survives where it is faster: the split-K kernel for a lone
// 32-channel output block, conv_wino4_kernel (wino4_kernel.hip; a split variant of THIS kernel measured 2 - 6 % slower there:
// tools/experiments/wino4r_split_variant.patch).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "device_util.h"
#include "wino4_lds_layout.h"

namespace ecseg {

// (timing-only ablations exist only in A/B builds, tools/w4r_variants.sh -DECSEG_W4R_ABL=<bits>: 1 no filter DMA, 2 no halo DMA, 4 no MFMAs;
// the hooks and their empty defaults: wino4_consts.inc, wino4_mfma_stage.inc)
#ifdef ECSEG_W4R_ABL
#define W4_DIAG_SKIP_HALO_DMA() do { if (ECSEG_W4R_ABL & 2) return; } while (0)
#define W4_DIAG_SKIP_FILTER_DMA() do { if (ECSEG_W4R_ABL & 1) return; } while (0)
#if ECSEG_W4R_ABL & 4
#define W4_MFMA(ACC, A, B) asm volatile("" :: "v"(A), "v"(B))
#endif
#endif
#include "wino4_consts.inc"
#define W4_HALO_RING 2
// raw image (only row_pass reads it): plain row / column order (one pad slot per row: W4Lds::RAW_ROW), the two 16-byte channel halves of a pixel next to each other
#define W4_HALO_SLOT(r, cc) const int h = (cc) & 1, hy = (r), hx = (cc) >> 1
#define W4_HALO_UPPER(cc) ((cc) & 1)
#define W4_HALO_L W4Lds::Raw
// filter stages (wino4_filter_dma.inc): wt4[nb][stage][wave] is 768 floats, the wave's double buffer follows the raw buffers and the t image
#define W4_FILTER_STRIDE (12 * 768 * 4)
#define W4_FILTER_LDS(buf) ((2 * W4_HS + W4R_TS + W4Lds::bw_stage(wave, buf)) * 16u)

namespace {
constexpr int W4R_TS = W4Lds::TS;       // slots of the t image: 2 regions x 6 transform rows x 4 tile rows x (18 columns x 2 channel halves), padded (wino4_lds_layout.h)
}

template <bool HEAD>
__global__ __launch_bounds__(768) void conv_wino4r_kernel(ConvParams p, int regs_x, int regs_y, int npairs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* Hs = reinterpret_cast<f32x4*>(smem);              // [2][W4_HS]        raw halo (group g -> buffer g & 1)
    f32x4* Ts = Hs + 2 * W4_HS;                              // [W4R_TS]          row-transformed halo of one group
    f32x4* Bs = Ts + W4R_TS;                                 // [12][2][W4_BWS]   per-wave filter stages

    const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xi = wave % 6, ch = wave / 6;
    const int li = lane & 31, lh = lane >> 5;

#include "wino4_region.inc"
    // ---- filter DMA: wt4[nb][stage][wave][point pair nu / 2][lane = h * 32 + cout][nu % 2][k 2], 768 floats per wave and stage ----
    const unsigned long long w_base = (unsigned long long)(size_t)(p.wt + ((size_t)nb * nstages * 12 + wave) * 768);
    f32x4* Bw = Bs + W4Lds::bw_stage(wave, 0);
#include "wino4_filter_dma.inc"

#include "wino4_lane_tile.inc"
    const int t_lane = W4Lds::t_lane(tg, xi, ty, lh, tx);      // the lane's tile in the t image

    f32x16 acc[6];
#pragma unroll
    for (int v = 0; v < 6; ++v)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[v][e] = 0.f;

#include "wino4_row_pass.inc"
    f32x4 t[6];
    auto load_t = [&]() __attribute__((always_inline)) {
        const f32x4* A = Ts + t_lane;
#pragma unroll
        for (int j = 0; j < 6; ++j) t[j] = A[W4Lds::t_col(j)];
    };
#include "wino4_mfma_stage.inc"
    // Per group g: barrier Y(g-1) (the t image holds group g, raw buffer g & 1 is free: this wave's two halo pieces of group g + 2 go out) and
    // barrier X(g) (nobody needs the t image of group g any more, the raw halo of group g + 1 has landed: row_pass(g + 1) follows).  The
    // three waves of a SIMD sit at different points of the sequence:
    //   class 0:   Y(g-1) | t <- image, S0(g)        | X(g) | row_pass(g+1), S1(g)
    //   class 1:   Y(g-1) | S1(g-1), t <- image      | X(g) | row_pass(g+1), S0(g)
    //   class 2:   Y(g-1) | t <- image, S0(g)        | X(g) | S1(g), row_pass(g+1)
    // Filter stage s = 2 g + ss lives in buffer ss and is streamed one stage ahead behind the MFMAs of the stage before.  Waits: the phase right behind Y has the two halo pieces issued behind Y younger than its stage -> vmcnt(2);
    // the other phase's stage is the youngest thing the wave issued -> vmcnt(0).  (Two stages ahead, as the split kernel streams: -1 %,
    // tools/experiments/wino4r_filter_two_stages_ahead.patch; s_setprio by rotation class, matrix phases above the transform: +-0.)
#define W4_S(ss, g, H) do { W4_SB(); if (H) W4_WAIT(2); else W4_WAIT(0); W4_SB(); \
                            mfma_stage(ss, ss, (ss) == 0 ? 2 * (g) + 1 : ((g) + 1 < ngroups ? 2 * (g) + 2 : 2 * (g)), -1); W4_SB(); } while (0)
    const int cls = wave >> 2;
    W4_HALO(0);
    if (ngroups > 1) W4_HALO(1);
    dma_filter_piece(0, 0, std::integral_constant<int, 0>{});
    dma_filter_piece(0, 0, std::integral_constant<int, 1>{});
    dma_filter_piece(0, 0, std::integral_constant<int, 2>{});
    if (ngroups > 1) W4_WAIT(5); else W4_WAIT(3);            // raw group 0 has landed
    W4_BARRIER();
    row_pass(0);
    if (cls == 0) {
        for (int grp = 0; grp < ngroups; ++grp) {
            W4_Y();
            const bool mh = grp + 2 < ngroups;
            if (mh) W4_HALO(grp + 2);
            load_t();
            W4_S(0, grp, mh);
            if (grp + 1 < ngroups) { W4_X(); row_pass(grp + 1); W4_SB(); }
            W4_S(1, grp, false);
        }
    } else if (cls == 1) {
        {
            W4_Y();
            const bool mh = 2 < ngroups;
            if (mh) W4_HALO(2);
            load_t();
            if (1 < ngroups) {
                if (mh) W4_WAIT(5); else W4_WAIT(3);         // raw group 1 has landed (this class has not waited for anything since the prologue)
                W4_X(); row_pass(1); W4_SB();
            }
            W4_S(0, 0, false);
        }
        for (int grp = 1; grp < ngroups; ++grp) {
            W4_Y();
            const bool mh = grp + 2 < ngroups;
            if (mh) W4_HALO(grp + 2);
            W4_S(1, grp - 1, mh);
            load_t();
            if (grp + 1 < ngroups) { W4_X(); row_pass(grp + 1); W4_SB(); }
            W4_S(0, grp, false);
        }
        W4_S(1, ngroups - 1, false);
    } else {
        for (int grp = 0; grp < ngroups; ++grp) {
            W4_Y();
            const bool mh = grp + 2 < ngroups;
            if (mh) W4_HALO(grp + 2);
            load_t();
            W4_S(0, grp, mh);
            if (grp + 1 < ngroups) { W4_X(); }
            W4_S(1, grp, false);
            if (grp + 1 < ngroups) { row_pass(grp + 1); W4_SB(); }
        }
    }
#undef W4_S

    // ---- output stage: two passes (channel halves) through a [xi][x][tile][32 couts] exchange image ----
#include "wino4_out_begin.inc"
    // fold the wave's own row (R = M[xi][:] A) into the exchange image
    auto write_R = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tl = (e & 3) + 8 * (e >> 2) + 4 * lh;               // accumulator row = tile slot
            const int fold_at = W4Lds::r_fold(xi, tl, li);
#include "wino4_fold.inc"
            o[W4Lds::r_plane(0)] = r0; o[W4Lds::r_plane(1)] = r1; o[W4Lds::r_plane(2)] = r2; o[W4Lds::r_plane(3)] = r3;
        }
    };
    if constexpr (!HEAD) {
        // Passes by TILE half instead of channel half (round 6): pass P takes the accumulator rows e = 8 P .. 8 P + 7 (tiles 16 P .. 16 P + 15) of ALL
        // 64 output channels, exchange image [xi][x][16 tiles][64 couts] - every wave folds and writes in BOTH passes (half as many rows each)
        // where the channel-half passes left six of the twelve waves waiting behind the other six's fold.  The same sums element by element:
        // bit-identical.  (Not for a fused head: its per-pixel class sums would then be spread over two waves.)
        const int cq = tid & 7, cx = (tid >> 3) & 3, nlo = (tid >> 5) & 1;          // channel quad, column of the tile, tile of the pair
        const int cwave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const float* rlane = Rs + W4Lds::r_comb_tile(cx, nlo, cq, 0, 0);     // (the function is a sum of a lane part and a unit part)
        const unsigned out_row = (unsigned)(W * p.out.cs);
        auto tile_pass = [&](auto pc) __attribute__((always_inline)) {
            constexpr int P = decltype(pc)::value;
            __syncthreads();                                 // main-loop LDS reads / previous pass's combine are done
#pragma unroll
            for (int e8 = 0; e8 < 8; ++e8) {
                const int e = 8 * P + e8;
                const int tl = (e8 & 3) + 8 * (e8 >> 2) + 4 * lh;         // tile slot within the half: 0..15
                const int fold_at = W4Lds::r_fold_tile(xi, tl, ch, li);
#include "wino4_fold.inc"
                o[W4Lds::r_plane(0)] = r0; o[W4Lds::r_plane(1)] = r1; o[W4Lds::r_plane(2)] = r2; o[W4Lds::r_plane(3)] = r3;
            }
            __syncthreads();
            if (P == 0) asm volatile("" :: "v"(bvp[0]), "v"(bvp[1]));      // (the bias wait in straight-line code: wino4_combine.inc)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int u = cwave + 12 * k;                // unit: tile pair u & 7 of this half x channel half u >> 3
                if (u >= 16) break;
                const int tp = u & 7, chh = u >> 3;
                const int nq8 = 4 * P + (tp >> 1);           // tile row pair index of the 32 tiles
                const int g = W4_QUAD_REGION(nq8), nty = nq8 >> 1;
                const int img = g ? r_img[1] : r_img[0];
                if (img < 0) continue;
                const int co = nb * 64 + chh * 32 + 4 * cq;
                if (co + 3 >= Cout) continue;                // (the missing channel half of a Cout % 64 == 32 block; wave-uniform per lane group: co_ok is all or nothing for chh)
                const f32x4 bv = chh ? bvp[1] : bvp[0];
                const float* r = rlane + W4Lds::r_comb_tile(0, 0, 0, tp, chh);
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(r);
                const f32x4 q1 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 1));
                const f32x4 q2 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 2));
                const f32x4 q3 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 3));
                const f32x4 q4 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 4));
                const f32x4 q5 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 5));
                const f32x4 s12 = q1 + q2, d12 = q1 - q2, s34 = q3 + q4, d34 = q3 - q4;
                // From here to the pool stores the item is wino4_combine.inc's, term for term.  It stays written out: one body included by both forms
                // is not byte-identical device code in this kernel (EXPERIMENTS.md round 11, tools/experiments/wino4_item_body.patch)
                f32x4 y[4];
                y[0] = q0 + s12 + s34 + bv;
                y[1] = KA * d12 + KB * d34 + bv;
                y[2] = KA2 * s12 + KB2 * s34 + bv;
                y[3] = KA3 * d12 + KB3 * d34 + q5 + bv;
                if (p.act == ECSEG_ACT_RELU) {
#pragma unroll
                    for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            float tv = y[yy][c];
                            asm("v_max_f32_e32 %0, 0, %1" : "=v"(tv) : "v"(tv));
                            y[yy][c] = tv;
                        }
                } else if (p.act != ECSEG_ACT_LINEAR) {
#pragma unroll
                    for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                        for (int c = 0; c < 4; ++c) y[yy][c] = apply_act_core(y[yy][c], p.act, p.alpha);
                }
                const int oy = (g ? r_y0[1] : r_y0[0]) + 4 * nty, ox = (g ? r_x0[1] : r_x0[0]) + 8 * (tp & 1);       // wave-uniform
                const unsigned out_lane = (unsigned)((4 * nlo + cx) * p.out.cs + co);
                float* ob = p.out.p + (((size_t)img * H + oy) * W + ox) * p.out.cs;
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
                    __builtin_nontemporal_store(y[yy], reinterpret_cast<f32x4*>(ob + (size_t)(out_lane + (unsigned)yy * out_row)));
                if (p.pool.p != nullptr) {                  // fused MaxPooling2D(2x2, stride 2), as in wino4_combine.inc
                    float* pb = p.pool.p + (((size_t)img * p.pool.h + (oy >> 1)) * p.pool.w + (ox >> 1)) * p.pool.cs;
                    const unsigned pool_lane = (unsigned)((2 * nlo + (cx >> 1)) * p.pool.cs + co);
#pragma unroll
                    for (int yp = 0; yp < 2; ++yp) {
                        f32x4 m;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float a = fmaxf(y[2 * yp][c], y[2 * yp + 1][c]);
                            m[c] = fmaxf(a, __shfl_xor(a, 8));
                        }
                        if (!(cx & 1)) *reinterpret_cast<f32x4*>(pb + (size_t)(pool_lane + (unsigned)(yp * p.pool.w * p.pool.cs))) = m;
                    }
                }
            }
        };
        tile_pass(std::integral_constant<int, 0>{});
        tile_pass(std::integral_constant<int, 1>{});
    } else
    for (int pass = 0; pass < 2; ++pass) {                   // fused head: passes by channel half
        __syncthreads();                                     // main-loop LDS reads / previous pass's combine are done
        if (ch == pass) write_R();
        __syncthreads();
#include "wino4_combine.inc"
    }
#include "wino4_head.inc"
}


bool conv_wino4r_supported(const ConvParams& p) { return conv_wino4_supported(p) && !(p.out.c == 32 && p.w4_split); }

hipError_t launch_conv_wino4r(const ConvParams& p, hipStream_t s) {
    if (p.head_w != nullptr && (!p.head_only || p.pool.p != nullptr)) return hipErrorInvalidValue;     // (the HEAD kernels write neither the features nor a pool)
    static DeviceOnce attr_set[2];                           // (per template instance)
    const int head = p.head_w != nullptr ? 1 : 0;
    return launch_wino4_grid(p, s, head ? conv_wino4r_kernel<true> : conv_wino4r_kernel<false>, attr_set[head],
                             (size_t)(2 * W4_HS + W4R_TS + 12 * 2 * W4_BWS) * 16, (p.out.c + 63) / 64);
}

}  // namespace ecseg
