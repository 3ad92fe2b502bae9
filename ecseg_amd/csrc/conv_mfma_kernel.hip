// The implicit-GEMM convolutions of the plan interpreter on the fp32 matrix cores of gfx950 (MI355X): conv_mfma_kernel and, for any
// taps / stride / dilation rate, conv_mfma_tap_kernel (below).  NHWC float32 everywhere.
//
// conv_mfma is an im2col-free implicit-GEMM convolution on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32, exact f32 fma chains).  Per workgroup: 128 output pixels (a TH x TW spatial tile of one
// patch) x BN output channels; the input halo tile and the filter slab of one 8-channel K-chunk are staged in LDS and
// every one of the R*S taps is served from that single staged halo (no im2col buffer, no re-read of the input).
//
//   M (MFMA rows)  = output pixels, lane i = l & 31 -> pixel i of the wave's 32-pixel strip
//   N (MFMA cols)  = output channels
//   K              = (tap, input channel); one MFMA consumes channels {e, 4 + e} of the chunk for one tap, so a
//                    single ds_read_b128 per operand feeds four MFMAs (k-order inside a chunk is permuted
//                    identically for A and B, which only re-orders the exact f32 accumulation).
//
// LDS images (conflict-free ds_read_b128: consecutive lanes read consecutive 16-byte slots)
//   As[half h][halo pixel][4 ch]           channels 4h .. 4h+3 of the chunk
//   Bs[tap][half h][out channel][4 ch]
// Global filter layout (re-laid out once at model load): wt[tap][chunk][h][N padded][4].
#include <cstdlib>

#include "common.h"
#include "device_util.h"

namespace ecseg {

template <int NT, int TW, int R, int S, int KCH = 1, int ST = 1>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvParams p, int tiles_x, int tiles_y, int nblk_n, int np_total) {
    // KCH = 8-channel K-chunks staged per barrier interval (4 for 1x1 taps: a single tap gives a wave only 4*NT MFMAs
    // per chunk, too few to amortise the barrier / staging cost).  ST = output stride (2: strided convolutions - the halo
    // tile covers (TH - 1) ST + R rows and a lane's A operand sits ST halo pixels from its neighbour's).
    constexpr int TH = 128 / TW;
    constexpr int HH = (TH - 1) * ST + R, HW = (TW - 1) * ST + S;
    constexpr int NPIX = HH * HW;
    constexpr int BN = NT * 32;
    constexpr int A_PIECES = NPIX * 2;
    constexpr int A_PER_T = (A_PIECES * KCH + 255) / 256;
    constexpr int B_PIECES = R * S * 2 * BN;
    constexpr int B_PER_T = (B_PIECES * KCH + 255) / 256;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* As = reinterpret_cast<f32x4*>(smem);   // [KCH][2][NPIX]
    f32x4* Bs = As + KCH * 2 * NPIX;              // [KCH][R*S][2][BN]

    const int tid = threadIdx.x;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int nb = bid % nblk_n; bid /= nblk_n;
    int tx0, ty0, img;
    if (p.lut != nullptr) {                                  // cropped launch: tile origins (in 4-pixel units) from the list
        const int i = bid / p.lut_len, v = p.lut[bid - i * p.lut_len];
        img = i * p.per_image + (v >> 16); ty0 = ((v >> 8) & 255) * 4; tx0 = (v & 255) * 4;
    } else {
        tx0 = (bid % tiles_x) * TW; bid /= tiles_x;
        ty0 = (bid % tiles_y) * TH; bid /= tiles_y;
        img = bid;
    }
    const int n0 = nb * BN;

    const int Hin = p.in.h, Win = p.in.w, Cin = p.in.c;
    const size_t in_img = (size_t)img * Hin * Win * p.in.cs;

    // ---- per-thread staging descriptors (fixed over the K loop) ----
    long a_off[A_PER_T];     // float offset of this thread's 16-byte piece for stage 0, or -1 when zero-filled
    int a_ch[A_PER_T];       // first channel of the piece inside stage 0
    int a_lds[A_PER_T];
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int q = tid + k * 256;
        a_off[k] = -1; a_lds[k] = -1; a_ch[k] = 0;
        if (q < A_PIECES * KCH) {
            const int kc = q / A_PIECES, qq = q - kc * A_PIECES;
            const int pix = qq >> 1, h = qq & 1;
            const int hy = pix / HW, hx = pix - hy * HW;
            const int iy = ty0 * ST - p.pad_top + hy, ix = tx0 * ST - p.pad_left + hx;
            a_lds[k] = (kc * 2 + h) * NPIX + pix;
            a_ch[k] = kc * 8 + h * 4;
            if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win)
                a_off[k] = (long)(in_img + ((size_t)iy * Win + ix) * p.in.cs + kc * 8 + h * 4);
        }
    }
    const size_t chunk_stride = (size_t)p.wt_chunk_stride;         // floats between consecutive chunks of one tap
    const size_t tap_stride = (size_t)p.wt_tap_stride;
    long b_off[B_PER_T];
    int b_kc[B_PER_T];
#pragma unroll
    for (int k = 0; k < B_PER_T; ++k) {
        const int q = tid + k * 256;
        b_off[k] = -1; b_kc[k] = 0;
        if (q < B_PIECES * KCH) {
            const int kc = q / B_PIECES, qq = q - kc * B_PIECES;
            const int tap = qq / (2 * BN), rem = qq - tap * 2 * BN;
            const int h = rem / BN, j = rem - h * BN;
            b_kc[k] = kc;
            b_off[k] = (long)(tap * tap_stride + kc * chunk_stride + ((size_t)h * np_total + n0 + j) * 4);
        }
    }
    const int nstages = (p.cin_chunks + KCH - 1) / KCH;

    f32x4 a_reg[A_PER_T], b_reg[B_PER_T];
    auto load_chunk = [&](int st) {
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (a_off[k] >= 0 && st * KCH * 8 + a_ch[k] < Cin)
                v = *reinterpret_cast<const f32x4*>(p.in.p + a_off[k] + (size_t)st * KCH * 8);
            a_reg[k] = v;
        }
#pragma unroll
        for (int k = 0; k < B_PER_T; ++k) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (b_off[k] >= 0 && st * KCH + b_kc[k] < p.cin_chunks)
                v = *reinterpret_cast<const f32x4*>(p.wt + b_off[k] + (size_t)st * KCH * chunk_stride);
            b_reg[k] = v;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k)
            if (a_lds[k] >= 0) As[a_lds[k]] = a_reg[k];
#pragma unroll
        for (int k = 0; k < B_PER_T; ++k) {
            const int q = tid + k * 256;
            if (q < B_PIECES * KCH) Bs[q] = b_reg[k];
        }
    };

    // ---- wave / lane roles ----
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    int ty, tx;
    if (TW == 32) { ty = wave; tx = li; } else { ty = 2 * wave + (li >> 4); tx = li & 15; }
    const f32x4* Ap = As + lh * NPIX + ty * ST * HW + tx * ST;
    const f32x4* Bp = Bs + lh * BN + li;

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;

    // Sub-pixel transposed convolutions (round 6): 7 of the 16 (tap, output phase) filter blocks of a 3x3 / stride-2 layer are all zero
    // - the phases have 4, 2, 2 and 1 taps - and the up-sample + 2x2 decoder step lowered to such a layer lives on exactly those 9.
    // skip[nt]: bit t set = tap t of this workgroup's 32-column tile nt multiplies zeros only (a tile that straddles two phases -
    // coutp = 16 - skips what both have in common).  Wave-uniform: one scalar branch per (tap, tile).
    unsigned skip[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        skip[nt] = 0;
        if (R == 2 && S == 2 && p.convt && p.tap_zero_mask) {
            const int ab0 = (n0 + nt * 32) / p.coutp, ab1 = min((n0 + nt * 32 + 31) / p.coutp, p.kT * p.kT - 1);
#pragma unroll
            for (int t = 0; t < R * S; ++t) {
                bool z = true;
                for (int ab = ab0; ab <= ab1; ++ab) z = z && ((p.tap_zero_mask >> (t * 4 + ab)) & 1);
                if (z) skip[nt] |= 1u << t;
            }
        }
    }

    load_chunk(0);
    for (int st = 0; st < nstages; ++st) {
        store_chunk();
        __syncthreads();
        if (st + 1 < nstages) load_chunk(st + 1);   // next stage's HBM/L2 latency hides under this stage's MFMAs
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const f32x4 a = Ap[kc * 2 * NPIX + r * HW + s];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if (R == 2 && S == 2 && ((skip[nt] >> (r * S + s)) & 1)) continue;
                        const f32x4 b = Bp[(kc * R * S + r * S + s) * 2 * BN + nt * 32];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[nt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- epilogue: each wave turns its 32 pixel x 32 channel accumulator tile around through a private 4-KB LDS tile
    //      (the K loop's last barrier has retired the staging buffers) so that a lane finishes 4 consecutive channels of
    //      one pixel: bias + activation, one 16-byte store; a wave instruction writes 8 pixels x 128 B instead of 64 x 4 B ----
    const int Hout = p.out.h, Wout = p.out.w, Cout = p.out.c;
    const int Ht = p.convt ? Hin + p.convt_ext : Hout, Wt = p.convt ? Win + p.convt_ext : Wout;   // extent the tiles walk over
    float* Xs = reinterpret_cast<float*>(smem) + wave * 1024;
    const bool vec_ok = (p.out.cs % 4 == 0) && (Cout % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.out.p) & 15) == 0);
    const int quad = lane & 7;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        int co = n0 + nt * 32 + 4 * quad, oa = 0, ob = 0;
        if (p.convt) {
            // N index = (a * kT + b) * coutp + co, decoded per lane: with coutp = 16 a 32-column tile holds BOTH column phases
            // b = 0, 1 of one row phase a, i.e. the two output pixels (2x, 2x + 1) a lane octet writes are neighbours in memory
            const int ab = co / p.coutp;
            co -= ab * p.coutp;
            oa = ab / p.kT; ob = ab - oa * p.kT;
            oa += p.phase_a; ob += p.phase_b;                  // (phase-by-phase launches: N holds one phase, ab = 0)
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) Xs[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + li] = acc[nt][e];
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias != nullptr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (co + c < Cout) bv[c] = p.bias[co + c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (lane >> 3) + 8 * r;               // pixel index inside the wave's 32-pixel strip
            f32x4 v = *reinterpret_cast<const f32x4*>(Xs + row * 32 + 4 * quad) + bv;
            v = apply_act4(v, p.act, p.alpha);
            int py, px;
            if (TW == 32) { py = wave; px = row; } else { py = 2 * wave + (row >> 4); px = row & 15; }
            const int tyy = ty0 + py, txx = tx0 + px;          // position in the tiled extent
            int oy = tyy, ox = txx;
            bool ok = tyy < Ht && txx < Wt;                     // the tile may overhang the extent
            if (p.convt) {
                oy = tyy * p.kT + oa - p.crop_top;
                ox = txx * p.kT + ob - p.crop_left;
                ok = ok && oy >= 0 && oy < Hout && ox >= 0 && ox < Wout;
            }
            if (ok) {
                float* o = p.out.p + (((size_t)img * Hout + oy) * Wout + ox) * p.out.cs + co;
                if (vec_ok && co + 3 < Cout) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(o));   // (streamed once, read by a later launch)
                else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) if (co + c < Cout) o[c] = v[c];
                }
            }
        }
    }
}

int conv_mfma_ntile(int cout) {
    if (cout % 128 == 0) return 128;
    if (cout % 64 == 0 || cout > 64) return 64;
    return 32;
}

bool conv_mfma_supported(const ConvParams& p) {
    const bool taps_ok = (p.R == 3 && p.S == 3) || (p.R == 2 && p.S == 2) || (p.R == 1 && p.S == 1) || (p.stride <= 1 && ((p.R == 2 && p.S == 1) || (p.R == 1 && p.S == 2)));
    const bool align_ok = (p.in.cs % 4 == 0) && (p.in.c % 4 == 0) && (((uintptr_t)p.in.p) % 16 == 0);
    return taps_ok && align_ok && p.in.c >= 8 && p.out.c >= 16;
}

template <int NT, int TW, int R, int S, int KCH = 1, int ST = 1>
static hipError_t launch_conv_mfma_t(const ConvParams& p, hipStream_t s) {
    constexpr int TH = 128 / TW;
    constexpr int BN = NT * 32;
    const int ext_h = p.convt ? p.in.h + p.convt_ext : p.out.h, ext_w = p.convt ? p.in.w + p.convt_ext : p.out.w;
    const int tiles_x = (ext_w + TW - 1) / TW, tiles_y = (ext_h + TH - 1) / TH;
    const int np_total = p.convt == 1 ? p.kT * p.kT * p.coutp : p.coutp;        // (convt == 2: one output phase per launch)
    const int nblk_n = np_total / BN;
    size_t lds = (size_t)KCH * (2 * ((TH - 1) * ST + R) * ((TW - 1) * ST + S) + R * S * 2 * BN) * 16;
    if (lds < 4 * 4096) lds = 4 * 4096;                       // the output stage needs a 4-KB exchange tile per wave
    const size_t grid = (p.lut != nullptr ? (size_t)(p.n / p.per_image) * p.lut_len : (size_t)p.n * tiles_x * tiles_y) * nblk_n;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv_mfma_kernel<NT, TW, R, S, KCH, ST>), dim3((unsigned)grid), dim3(256), lds, s, p, tiles_x, tiles_y,
                       nblk_n, np_total);
    return hipGetLastError();
}

template <int NT, int TW>
static hipError_t launch_conv_mfma_rs(const ConvParams& p, hipStream_t s) {
    if (p.stride == 2 && !p.convt) {                          // strided halo gather (classifier stems, down-sampling convolutions)
        if (p.R == 3) return launch_conv_mfma_t<NT, TW, 3, 3, 1, 2>(p, s);
        if (p.R == 2) return launch_conv_mfma_t<NT, TW, 2, 2, 1, 2>(p, s);
        return launch_conv_mfma_t<NT, TW, 1, 1, 2, 2>(p, s);
    }
    if (p.R == 3) return launch_conv_mfma_t<NT, TW, 3, 3>(p, s);
    if (p.R == 2 && p.S == 2) return launch_conv_mfma_t<NT, TW, 2, 2>(p, s);
    if (p.R == 2 && p.S == 1) return launch_conv_mfma_t<NT, TW, 2, 1, 2>(p, s);     // (the two-tap phases of a 3x3 / stride-2 transposed convolution)
    if (p.R == 1 && p.S == 2) return launch_conv_mfma_t<NT, TW, 1, 2, 2>(p, s);
    return launch_conv_mfma_t<NT, TW, 1, 1, 2>(p, s);      // K-chunks per barrier: 1 / 2 / 4 / 8 measured 0 / +0.2 / -0.2 / -1.5 % (A/B)
}

hipError_t launch_conv_mfma(const ConvParams& p, hipStream_t s) {
    // transposed convolutions whose kT x kT phases x padded channels fit one 128-column tile (Cout <= 32 at 2x2): ONE workgroup
    // computes every output phase of its input tile - the tile is staged once instead of once per phase, and the per-thread
    // staging descriptors / prologue of these short-K layers are amortised over 2 - 4x the work
    const int np_t = p.convt == 1 ? p.kT * p.kT * p.coutp : 0;
    const int bn = (p.convt && np_t <= 128 && np_t % 32 == 0) ? np_t : conv_mfma_ntile(p.out.c);
    const bool wide = p.force_tw ? p.force_tw == 32 : (p.convt ? p.in.w : p.out.w) >= 32;
    if (bn == 128) return wide ? launch_conv_mfma_rs<4, 32>(p, s) : launch_conv_mfma_rs<4, 16>(p, s);
    if (bn == 64) return wide ? launch_conv_mfma_rs<2, 32>(p, s) : launch_conv_mfma_rs<2, 16>(p, s);
    return wide ? launch_conv_mfma_rs<1, 32>(p, s) : launch_conv_mfma_rs<1, 16>(p, s);
}

// ------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution, tap by tap.  Workgroup = 128 output pixels (TH x TW tile of one patch) x BN output channels,
// as conv_mfma_kernel (above), but the K loop walks (tap, group of KCH 8-channel chunks) and stages, per step,
// the 128 input pixels THAT tap reads: pixel (oy * stride - pad + r * dil, ox * stride - pad + s * dil).  With a dilation
// rate of 6 - 18 (ASPP heads) the union of the taps' footprints is (TH + 2 dil) x (TW + 2 dil) pixels of which every tap
// uses 128: a shared halo would not fit LDS and would be read once per tap anyway.  Input re-reads (R * S times) are served
// by L2; the MFMA work per staged byte equals the 1x1 kernel's.
//
//   M = output pixels (lane & 31 -> pixel of the wave's 32-pixel strip), N = output channels, K = (tap, input channel);
//   one MFMA (v_mfma_f32_32x32x2_f32) consumes channels {e, 4 + e} of a chunk, so one ds_read_b128 per operand feeds four.
// LDS: As[kc][half][128 pixels][4 ch], Bs[kc][half][BN][4 ch]; global filter layout = relayout_conv (filter_layout.hip):
// wt[tap][chunk][half][N padded][4].
// ------------------------------------------------------------------------------------------------------------
template <int NT, int TW>
__global__ __launch_bounds__(256) void conv_mfma_tap_kernel(ConvParams p, int tiles_x, int tiles_y, int nblk_n, int dil) {
    constexpr int KCH = 4;
    constexpr int BN = NT * 32;
    constexpr int B_PER_T = (2 * BN * KCH) / 256;            // = NT

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* As = reinterpret_cast<f32x4*>(smem);              // [KCH][2][128]
    f32x4* Bs = As + KCH * 2 * 128;                          // [KCH][2][BN]

    const int tid = threadIdx.x;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int nb = bid % nblk_n; bid /= nblk_n;
    const int tx0 = (bid % tiles_x) * TW; bid /= tiles_x;
    const int ty0 = (bid % tiles_y) * (128 / TW); bid /= tiles_y;
    const int img = bid;
    const int n0 = nb * BN;
    const int Hin = p.in.h, Win = p.in.w, Cin = p.in.c;
    const int st = p.stride > 0 ? p.stride : 1;
    const size_t in_img = (size_t)img * Hin * Win * p.in.cs;

    // this thread's A piece: pixel a_pix of the tile, channel half a_h, for every one of the KCH chunks of a step
    const int a_pix = tid >> 1, a_h = tid & 1;
    const int a_iy0 = (ty0 + a_pix / TW) * st - p.pad_top, a_ix0 = (tx0 + a_pix % TW) * st - p.pad_left;
    const size_t chunk_stride = (size_t)p.wt_chunk_stride, tap_stride = (size_t)p.wt_tap_stride;
    // B pieces: q = tid + k * 256 over [kc][half][BN]
    const int ngrp = (p.cin_chunks + KCH - 1) / KCH;
    const int nsteps = p.R * p.S * ngrp;

    f32x4 a_reg[KCH], b_reg[B_PER_T];
    auto load_step = [&](int step) {
        const int tap = step / ngrp, grp = step - tap * ngrp;
        const int r = tap / p.S, s = tap - r * p.S;
        const int iy = a_iy0 + r * dil, ix = a_ix0 + s * dil;
        const bool inside = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
        const float* ap = p.in.p + in_img + ((size_t)(inside ? iy : 0) * Win + (inside ? ix : 0)) * p.in.cs + a_h * 4;
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
            const int ch = (grp * KCH + kc) * 8 + a_h * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (inside && ch < Cin) v = *reinterpret_cast<const f32x4*>(ap + (grp * KCH + kc) * 8);
            a_reg[kc] = v;
        }
#pragma unroll
        for (int k = 0; k < B_PER_T; ++k) {
            const int q = tid + k * 256;
            const int kc = q / (2 * BN), rem = q - kc * 2 * BN;
            const int h = rem / BN, j = rem - h * BN;
            const int chunk = grp * KCH + kc;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (chunk < p.cin_chunks)
                v = *reinterpret_cast<const f32x4*>(p.wt + tap * tap_stride + chunk * chunk_stride + ((size_t)h * p.coutp + n0 + j) * 4);
            b_reg[k] = v;
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) As[(kc * 2 + a_h) * 128 + a_pix] = a_reg[kc];
#pragma unroll
        for (int k = 0; k < B_PER_T; ++k) Bs[tid + k * 256] = b_reg[k];
    };

    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const f32x4* Ap = As + lh * 128 + wave * 32 + li;        // (row-major TH x TW tile: pixel index = wave * 32 + li for both tile shapes)
    const f32x4* Bp = Bs + lh * BN + li;

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;

    load_step(0);
    for (int step = 0; step < nsteps; ++step) {
        store_step();
        __syncthreads();
        if (step + 1 < nsteps) load_step(step + 1);
        const int grp = step % ngrp;
        const int live = min(KCH, p.cin_chunks - grp * KCH);   // chunks of this step that exist (uniform)
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
            if (kc < live) {
                const f32x4 a = Ap[kc * 2 * 128];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f32x4 b = Bp[kc * 2 * BN + nt * 32];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[nt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // output stage: every wave turns its 32 x 32 accumulator tile around through a private 4-KB LDS tile so that a lane
    // finishes 4 consecutive channels of one pixel (bias, activation, one 16-byte store)
    const int Hout = p.out.h, Wout = p.out.w, Cout = p.out.c;
    float* Xs = reinterpret_cast<float*>(smem) + wave * 1024;
    const bool vec_ok = (p.out.cs % 4 == 0) && (Cout % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.out.p) & 15) == 0);
    const int quad = lane & 7;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + nt * 32 + 4 * quad;
#pragma unroll
        for (int e = 0; e < 16; ++e) Xs[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + li] = acc[nt][e];
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias != nullptr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (co + c < Cout) bv[c] = p.bias[co + c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (lane >> 3) + 8 * r;               // pixel inside the wave's 32-pixel strip
            f32x4 v = *reinterpret_cast<const f32x4*>(Xs + row * 32 + 4 * quad) + bv;
            v = apply_act4(v, p.act, p.alpha);
            const int pix = wave * 32 + row;
            const int oy = ty0 + pix / TW, ox = tx0 + pix % TW;
            if (oy < Hout && ox < Wout) {
                float* o = p.out.p + (((size_t)img * Hout + oy) * Wout + ox) * p.out.cs + co;
                if (vec_ok && co + 3 < Cout) *reinterpret_cast<f32x4*>(o) = v;
                else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) if (co + c < Cout) o[c] = v[c];
                }
            }
        }
    }
}

bool conv_mfma_tap_supported(const ConvParams& p) {
    return (p.in.cs % 4 == 0) && (p.in.c % 4 == 0) && ((((uintptr_t)p.in.p) & 15) == 0) && p.in.c >= 8 && p.R >= 1 && p.S >= 1;
}

template <int NT, int TW>
static hipError_t launch_conv_mfma_tap_t(const ConvParams& p, int dil, hipStream_t s) {
    constexpr int TH = 128 / TW, BN = NT * 32;
    const int tiles_x = (p.out.w + TW - 1) / TW, tiles_y = (p.out.h + TH - 1) / TH;
    const int nblk_n = p.coutp / BN;
    size_t lds = (size_t)4 * (2 * 128 + 2 * BN) * 16;
    if (lds < 4 * 4096) lds = 4 * 4096;
    const size_t grid = (size_t)p.n * tiles_x * tiles_y * nblk_n;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv_mfma_tap_kernel<NT, TW>), dim3((unsigned)grid), dim3(256), lds, s, p, tiles_x, tiles_y, nblk_n, dil);
    return hipGetLastError();
}

hipError_t launch_conv_mfma_tap(const ConvParams& p, int dil, hipStream_t s) {
    if (dil < 1) dil = 1;
    const int bn = conv_mfma_ntile(p.out.c);
    if (p.coutp % bn != 0) return hipErrorInvalidValue;
    const bool wide = p.out.w >= 32;
    if (bn == 128) return wide ? launch_conv_mfma_tap_t<4, 32>(p, dil, s) : launch_conv_mfma_tap_t<4, 16>(p, dil, s);
    if (bn == 64) return wide ? launch_conv_mfma_tap_t<2, 32>(p, dil, s) : launch_conv_mfma_tap_t<2, 16>(p, dil, s);
    return wide ? launch_conv_mfma_tap_t<1, 32>(p, dil, s) : launch_conv_mfma_tap_t<1, 16>(p, dil, s);
}

}  // namespace ecseg
