// Winograd F(2x2,3x3) convolutions of the plan interpreter for gfx950 (MI355X): conv_wino_kernel and, for narrow layers, the
// filter-resident conv_wino_res_kernel.  NHWC float32 views (common.h: TView).
#include "common.h"
#include "device_util.h"

namespace ecseg {

// ------------------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) on the fp32 matrix cores: 16 instead of 36 multiplies per 2x2 output block (2.25x fewer MFMAs).
//
//   Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A        d: 4x4 input tile, g: 3x3 filter, Y: 2x2 outputs
//
// The filter transform U = G g G^T is done once at model load (float64 on the host).  A workgroup owns 4 x 8 tiles
// (8 x 16 output pixels) x BN output channels; its four waves split the 16 transform points by ROW a of the 4x4
// transform domain: wave a reads the two raw input rows its row transform needs straight from the staged halo in LDS,
// forms t = B^T[a,:] d and the four column points V[a][0..3] in registers (32 packed adds per 32 MFMAs - free beside
// the matrix pipe) and multiplies them with U[a][b] on the MFMA.  No transformed input ever touches LDS or HBM.
// After the K loop each wave folds its own row (R_a = M[a][:] A) in registers, the four rows meet once through LDS,
// and Y = A^T R (+ bias, activation) is written as 128-byte row segments.
//
// LDS: As[h][col parity][10 rows][12 (9 used)][4ch] - even / odd halo columns in separate planes and a row pitch of
// 12 slots make every ds_read_b128 of the 4 x 8 tile lanes conflict-free; Bs[point 16][h][BN][4ch].
// Winograd output stage shared by the kernels below.  The four waves (transform rows a = 0..3) of a row tile fold
// their own row in registers (R_a = M[a][:] A), meet through LDS in a [a][jp][tile][channel] image, and every lane then
// finishes 4 consecutive output channels of one pixel pair: Y = A^T R + bias, activation, two 16-byte stores.  A wave
// instruction writes 4 pixels x 256 B: 8 store instructions per wave instead of 64 dword stores.
template <int NT>
__device__ __forceinline__ void wino_write_R(float* Rs, const f32x16 (&acc)[4][NT], int wa, int lane) {
    constexpr int BN = NT * 32;
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = (e & 3) + 8 * (e >> 2) + 4 * lh;           // accumulator row = tile index inside the row tile
            const float ra = acc[0][nt][e] + acc[1][nt][e] + acc[2][nt][e];
            const float rb = acc[1][nt][e] - acc[2][nt][e] - acc[3][nt][e];
            Rs[((wa * 2 + 0) * 32 + t) * BN + nt * 32 + li] = ra;
            Rs[((wa * 2 + 1) * 32 + t) * BN + nt * 32 + li] = rb;
        }
}

template <int NT>
__device__ __forceinline__ void wino_store_Y(const float* Rs, const ConvParams& p, int img, int oy0, int ox0, int n0, int wa,
                                             int lane) {
    constexpr int BN = NT * 32;
    constexpr int QN = BN / 4;                 // channel quads per pixel
    constexpr int TPI = 64 / QN;               // tiles per wave instruction
    const int q = lane % QN, tsub = lane / QN;
    const int Hout = p.out.h, Wout = p.out.w, Cout = p.out.c;
    const int co = n0 + 4 * q;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && co + 3 < Cout) bv = *reinterpret_cast<const f32x4*>(p.bias + co);
    f32x4 pm = {0.f, 0.f, 0.f, 0.f};
    // 32 tiles x 2 column parities, 4 waves x TPI tiles per step; a wave does both column parities of its tiles (the
    // fused 2x2 max-pool below needs the 2 x 2 outputs of a tile in one thread)
    for (int it = 2 * wa; it < (32 / TPI) * 2; it += (it & 1) ? 7 : 1) {
        const int jp = it & 1, t = (it >> 1) * TPI + tsub;
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(Rs + ((0 * 2 + jp) * 32 + t) * BN + 4 * q);
        const f32x4 q1 = *reinterpret_cast<const f32x4*>(Rs + ((1 * 2 + jp) * 32 + t) * BN + 4 * q);
        const f32x4 q2 = *reinterpret_cast<const f32x4*>(Rs + ((2 * 2 + jp) * 32 + t) * BN + 4 * q);
        const f32x4 q3 = *reinterpret_cast<const f32x4*>(Rs + ((3 * 2 + jp) * 32 + t) * BN + 4 * q);
        f32x4 y0 = q0 + q1 + q2 + bv, y1 = q1 - q2 - q3 + bv;
        y0 = apply_act4(y0, p.act, p.alpha); y1 = apply_act4(y1, p.act, p.alpha);
        const int oy = oy0 + 2 * (t >> 3), ox = ox0 + 2 * (t & 7) + jp;
        if (co + 3 < Cout && ox < Wout) {
            float* o = p.out.p + (((size_t)img * Hout + oy) * Wout + ox) * p.out.cs + co;
            if (oy < Hout) *reinterpret_cast<f32x4*>(o) = y0;
            if (oy + 1 < Hout) *reinterpret_cast<f32x4*>(o + (size_t)Wout * p.out.cs) = y1;
        }
        if (p.pool.p != nullptr) {
            // fused MaxPooling2D(2x2, stride 2): even extents (checked by the caller), so a tile is inside or outside as a whole
#pragma unroll
            for (int c = 0; c < 4; ++c) pm[c] = jp ? fmaxf(pm[c], fmaxf(y0[c], y1[c])) : fmaxf(y0[c], y1[c]);
            if (jp && co + 3 < Cout && ox < Wout && oy + 1 < Hout)
                *reinterpret_cast<f32x4*>(p.pool.p + (((size_t)img * p.pool.h + (oy >> 1)) * p.pool.w + (ox >> 1)) * p.pool.cs + co) = pm;
        }
    }
}

template <int NT, int MT>
__global__ __launch_bounds__(256, (MT == 1 ? 2 : 1)) void conv_wino_kernel(ConvParams p, int tiles_x, int tiles_y, int nblk_n) {
    constexpr int TTY = 4 * MT, TTX = 8;                     // MT MFMA row tiles of 4 x 8 Winograd tiles each
    constexpr int HR = 2 * TTY + 2, HC = 2 * TTX + 2;       // halo: (8 MT + 2) x 18 pixels
    constexpr int CS = 12;                                   // slots per (plane, row): 9 used
    constexpr int PLANE = HR * CS;
    constexpr int A_SLOTS = 4 * PLANE;                       // [h][parity]
    constexpr int BN = NT * 32;
    constexpr int A_PIECES = HR * HC * 2;
    constexpr int A_PER_T = (A_PIECES + 255) / 256;
    constexpr int B_PIECES = 16 * 2 * BN;
    constexpr int B_PER_T = B_PIECES / 256;

    // double-buffered: [As0 | As1 | Bs0 | Bs1]; the filter slab goes global -> LDS directly (LDS-DMA, no VGPR staging)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* As = reinterpret_cast<f32x4*>(smem);
    f32x4* Bs = As + 2 * A_SLOTS;

    const int tid = threadIdx.x;
    // spatial position fastest, output-channel block slowest: the workgroups that run together on one XCD stream the
    // same filter slabs
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int bx = bid % tiles_x; bid /= tiles_x;
    const int by = bid % tiles_y; bid /= tiles_y;
    const int img = bid % p.n; bid /= p.n;
    const int nb = bid;
    const int ox0 = bx * (2 * TTX), oy0 = by * (2 * TTY);
    const int n0 = nb * BN;
    const int Hin = p.in.h, Win = p.in.w, Cin = p.in.c;
    const size_t in_img = (size_t)img * Hin * Win * p.in.cs;

    // rows / columns this window may read (ConvParams::in_box; the whole image otherwise): zero outside
    int lo_y = 0, hi_y = Hin - 1, lo_x = 0, hi_x = Win - 1;
    if (p.in_box != nullptr) {
        const int32_t* bx = p.in_box + 4 * ((img + p.box_first) % p.per_image);
        lo_y = bx[0]; hi_y = bx[1]; lo_x = bx[2]; hi_x = bx[3];
    }
    long a_off[A_PER_T];
    int a_ch[A_PER_T], a_lds[A_PER_T];
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int q = tid + k * 256;
        a_off[k] = -1; a_lds[k] = -1; a_ch[k] = 0;
        if (q < A_PIECES) {
            const int pix = q >> 1, h = q & 1;
            const int hy = pix / HC, hx = pix - hy * HC;
            const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
            a_lds[k] = (h * 2 + (hx & 1)) * PLANE + hy * CS + (hx >> 1);
            a_ch[k] = h * 4;
            if (iy >= lo_y && iy <= hi_y && ix >= lo_x && ix <= hi_x)
                a_off[k] = (long)(in_img + ((size_t)iy * Win + ix) * p.in.cs + h * 4);
        }
    }
    const size_t chunk_stride = (size_t)p.wt_chunk_stride;
    const size_t tap_stride = (size_t)p.wt_tap_stride;
    long b_off[B_PER_T];
#pragma unroll
    for (int k = 0; k < B_PER_T; ++k) {
        const int q = tid + k * 256;
        const int tap = q / (2 * BN), rem = q - tap * 2 * BN;
        const int h = rem / BN, j = rem - h * BN;
        b_off[k] = (long)(tap * tap_stride + ((size_t)h * p.coutp + n0 + j) * 4);
    }
    f32x4 a_reg[A_PER_T];
    auto load_a = [&](int c) {
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (a_off[k] >= 0 && c * 8 + a_ch[k] < Cin)
                v = *reinterpret_cast<const f32x4*>(p.in.p + a_off[k] + (size_t)c * 8);
            a_reg[k] = v;
        }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k)
            if (a_lds[k] >= 0) As[buf * A_SLOTS + a_lds[k]] = a_reg[k];
    };
    auto dma_b = [&](int c, int buf) {          // LDS destination = wave base + lane * 16: the slab image is lane-linear
#pragma unroll
        for (int k = 0; k < B_PER_T; ++k) {
            const float* g = p.wt + b_off[k] + (size_t)c * chunk_stride;
            typedef const __attribute__((address_space(1))) void* gptr_t;
            typedef __attribute__((address_space(3))) void* lptr_t;
            __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(Bs + buf * B_PIECES + tid + k * 256), 16, 0, 0);
        }
    };

    const int lane = tid & 63, wa = tid >> 6;              // wave = transform row a
    const int li = lane & 31, lh = lane >> 5;
    const int ti = li >> 3, tj = li & 7;
    // row transform of wave a: t = s0 * d[r0] + s1 * d[r1]
    const int r0 = (wa == 0) ? 0 : 1, r1 = (wa == 3) ? 3 : 2;
    const float s0 = (wa == 2) ? -1.f : 1.f, s1 = (wa == 0 || wa == 3) ? -1.f : 1.f;
    const int a0_off = (lh * 2) * PLANE + (2 * ti + r0) * CS + tj;         // even columns (j = 0, 2)
    const int a1_off = (lh * 2) * PLANE + (2 * ti + r1) * CS + tj;
    const int b_lane = (wa * 4 * 2 + lh) * BN + li;

    f32x16 acc[MT][4][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][b][nt][e] = 0.f;

    load_a(0);
    dma_b(0, 0);
    store_a(0);
    __syncthreads();                                       // (hipcc drains vmcnt before the barrier: slab 0 has landed)
    for (int c = 0; c < p.cin_chunks; ++c) {
        const int cur = c & 1;
        const bool more = c + 1 < p.cin_chunks;
        if (more) { load_a(c + 1); dma_b(c + 1, cur ^ 1); }   // next chunk streams in under this chunk's MFMAs
        const f32x4* A0 = As + cur * A_SLOTS + a0_off;
        const f32x4* A1 = As + cur * A_SLOTS + a1_off;
        const f32x4* Bp = Bs + cur * B_PIECES + b_lane;
        // issue the LDS reads of the chunk first (8 halo fragments per row tile + 4*NT filter fragments), then
        // transform, then 32*MT MFMAs back to back; the second row tile's transform overlaps the first one's MFMAs
        f32x4 d[MT][8];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int ro = m * 8 * CS;                     // row tile m starts 8 halo rows further down
            d[m][0] = A0[ro]; d[m][1] = A1[ro]; d[m][2] = A0[ro + PLANE]; d[m][3] = A1[ro + PLANE];
            d[m][4] = A0[ro + 1]; d[m][5] = A1[ro + 1]; d[m][6] = A0[ro + PLANE + 1]; d[m][7] = A1[ro + PLANE + 1];
        }
        f32x4 w[4][NT];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w[b][nt] = Bp[b * 2 * BN + nt * 32];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            // halo column j of the tile: plane (j & 1), slot + (j >> 1)
            const f32x4 t0 = s0 * d[m][0] + s1 * d[m][1];
            const f32x4 t1 = s0 * d[m][2] + s1 * d[m][3];
            const f32x4 t2 = s0 * d[m][4] + s1 * d[m][5];
            const f32x4 t3 = s0 * d[m][6] + s1 * d[m][7];
            f32x4 V[4];
            V[0] = t0 - t2; V[1] = t1 + t2; V[2] = t2 - t1; V[3] = t1 - t3;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc[m][b][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[b][e], w[b][nt][e], acc[m][b][nt], 0, 0, 0);
                }
            }
        }
        if (more) store_a(cur ^ 1);
        __syncthreads();
    }

    // ---- output stage, one row tile at a time (wino_write_R / wino_store_Y) ----
    float* Rs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m) __syncthreads();
        wino_write_R<NT>(Rs, acc[m], wa, lane);
        __syncthreads();
        wino_store_Y<NT>(Rs, p, img, oy0 + 8 * m, ox0, n0, wa, lane);
    }
}

template <int NT, int MT>
static hipError_t launch_conv_wino_t(const ConvParams& p, hipStream_t s) {
    constexpr int BN = NT * 32;
    constexpr int TTY = 4 * MT;
    const int tiles_x = (p.out.w + 15) / 16, tiles_y = (p.out.h + 2 * TTY - 1) / (2 * TTY);
    const int nblk_n = p.coutp / BN;
    size_t lds = (size_t)2 * (4 * (2 * TTY + 2) * 12 + 16 * 2 * BN) * 16;
    const size_t lds_epi = (size_t)4 * 2 * NT * 4 * 64 * 16;
    if (lds_epi > lds) lds = lds_epi;
    const size_t grid = (size_t)p.n * tiles_x * tiles_y * nblk_n;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    static DeviceOnce attr_set;                             // the attribute is per device
    const hipError_t ea = attr_set.run([&] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_wino_kernel<NT, MT>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL((conv_wino_kernel<NT, MT>), dim3((unsigned)grid), dim3(256), lds, s, p, tiles_x, tiles_y, nblk_n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------
// Filter-resident F(2x2, 3x3) for NARROW layers (Cin <= 32, Cout <= 32: the full-resolution levels of base-16 / base-32
// U-Nets).  conv_wino_kernel streams a 16-point filter slab per 8 input channels for every 8 x 16 output pixels; with
// <= 32 channels that slab (16 KB) is larger than the input tile it is multiplied with, and the layer runs at the
// filter stream's L2 rate (1.6 TB/s of HBM-side traffic, 0.16-0.23 of the MFMA peak).  Here the whole transformed
// filter of a wave's transform row (4 points x Cin x 32 output channels = 16 * CH registers) is loaded ONCE into
// registers and the workgroup walks `tpw` tiles of a tile row: per tile only the input halo (all channels, one LDS
// image) and the outputs move.  Same arithmetic, lane maps and output stage as conv_wino_kernel<1, 1> (bit-identical
// results): wave a = transform row a, 32 MFMAs per 8 input channels and tile.
// Pipeline per tile (two barriers): the next tile's halo is fetched into registers before the MFMAs of the current one,
// stored to LDS after the exchange barrier (the halo image is dead by then) and before the output stores are issued.
// ------------------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256, 2) void conv_wino_res_kernel(ConvParams p, int tiles_x, int tiles_y, int segs_x, int tpw) {
    constexpr int HR = 10, HC = 18;                          // halo of 4 x 8 Winograd tiles: 10 x 18 pixels
    constexpr int CS = 12;                                   // slots per (plane, row): 9 used
    constexpr int PLANE = HR * CS;
    constexpr int A_SLOTS = 4 * PLANE;                       // per 8-channel chunk: [h][column parity]
    constexpr int PIECES = HR * HC * 2 * CH;                 // 16-byte pieces of one halo (all channels)
    constexpr int A_PER_T = (PIECES + 255) / 256;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* As = reinterpret_cast<f32x4*>(smem);              // [CH][A_SLOTS]
    float* Rs = reinterpret_cast<float*>(As + CH * A_SLOTS); // [4][2][32][32] output exchange image

    const int tid = threadIdx.x;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int seg = bid % segs_x; bid /= segs_x;
    const int by = bid % tiles_y; bid /= tiles_y;
    const int img = bid;
    const int bx0 = seg * tpw;
    const int ntile = min(tpw, tiles_x - bx0);
    const int oy0 = by * 8;
    const int Hin = p.in.h, Win = p.in.w, Cin = p.in.c;
    const size_t in_img = (size_t)img * Hin * Win * p.in.cs;

    // rows / columns this window may read (ConvParams::in_box; the whole image otherwise): zero outside
    int lo_y = 0, hi_y = Hin - 1, lo_x = 0, hi_x = Win - 1;
    if (p.in_box != nullptr) {
        const int32_t* bx = p.in_box + 4 * ((img + p.box_first) % p.per_image);
        lo_y = bx[0]; hi_y = bx[1]; lo_x = bx[2]; hi_x = bx[3];
    }
    // halo pieces of this thread: consecutive threads take the 2 * CH channel quads of one pixel (Cin * 4 contiguous bytes)
    long a_off[A_PER_T];                                     // offset of the piece for tile column 0 (may be "negative" at x = -1)
    int a_lds[A_PER_T], a_hx[A_PER_T];                       // LDS slot (-1: no piece), halo column | 0x100 when the row / channels are outside
#pragma unroll
    for (int k = 0; k < A_PER_T; ++k) {
        const int q = tid + k * 256;
        a_off[k] = 0; a_lds[k] = -1; a_hx[k] = 0x100;
        if (q < PIECES) {
            const int pix = q / (2 * CH), sub = q - pix * (2 * CH);
            const int c = sub >> 1, h = sub & 1;
            const int hy = pix / HC, hx = pix - hy * HC;
            const int iy = oy0 - 1 + hy;
            a_lds[k] = c * A_SLOTS + (h * 2 + (hx & 1)) * PLANE + hy * CS + (hx >> 1);
            const bool ok = iy >= lo_y && iy <= hi_y && c * 8 + h * 4 < Cin;
            a_hx[k] = hx | (ok ? 0 : 0x100);
            a_off[k] = (long)in_img + ((long)iy * Win + (long)(bx0 * 16 - 1 + hx)) * p.in.cs + c * 8 + h * 4;
        }
    }
    f32x4 a_reg[A_PER_T];
    auto load_a = [&](int t) {                               // tile t of this workgroup's walk
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int ix = (bx0 + t) * 16 - 1 + (a_hx[k] & 0xff);
            if (!(a_hx[k] & 0x100) && ix >= lo_x && ix <= hi_x)
                v = *reinterpret_cast<const f32x4*>(p.in.p + a_off[k] + (long)t * 16 * p.in.cs);
            a_reg[k] = v;
        }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int k = 0; k < A_PER_T; ++k)
            if (a_lds[k] >= 0) As[a_lds[k]] = a_reg[k];
    };

    const int lane = tid & 63, wa = tid >> 6;                // wave = transform row a
    const int li = lane & 31, lh = lane >> 5;
    const int ti = li >> 3, tj = li & 7;
    const int r0 = (wa == 0) ? 0 : 1, r1 = (wa == 3) ? 3 : 2;
    const float s0 = (wa == 2) ? -1.f : 1.f, s1 = (wa == 0 || wa == 3) ? -1.f : 1.f;
    const int a0_off = (lh * 2) * PLANE + (2 * ti + r0) * CS + tj;
    const int a1_off = (lh * 2) * PLANE + (2 * ti + r1) * CS + tj;

    load_a(0);
    // the wave's filter fragments: [chunk][column point b]: 4 k-steps of the MFMA B operand (lane = (channel half lh, cout li))
    f32x4 w[CH][4];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            w[c][b] = *reinterpret_cast<const f32x4*>(p.wt + (size_t)(wa * 4 + b) * (size_t)p.wt_tap_stride +
                                                      (size_t)c * (size_t)p.wt_chunk_stride + ((size_t)lh * p.coutp + li) * 4);
    store_a();
    __syncthreads();

    for (int t = 0; t < ntile; ++t) {
        const bool more = t + 1 < ntile;
        if (more) load_a(t + 1);                             // lands under this tile's MFMAs
        f32x16 acc[4][1];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[b][0][e] = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const f32x4* A0 = As + c * A_SLOTS + a0_off;
            const f32x4* A1 = As + c * A_SLOTS + a1_off;
            const f32x4 d0 = A0[0], d1 = A1[0], d2 = A0[PLANE], d3 = A1[PLANE];
            const f32x4 d4 = A0[1], d5 = A1[1], d6 = A0[PLANE + 1], d7 = A1[PLANE + 1];
            const f32x4 t0 = s0 * d0 + s1 * d1;
            const f32x4 t1 = s0 * d2 + s1 * d3;
            const f32x4 t2 = s0 * d4 + s1 * d5;
            const f32x4 t3 = s0 * d6 + s1 * d7;
            f32x4 V[4];
            V[0] = t0 - t2; V[1] = t1 + t2; V[2] = t2 - t1; V[3] = t1 - t3;
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[b][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[b][e], w[c][b][e], acc[b][0], 0, 0, 0);
        }
        wino_write_R<1>(Rs, acc, wa, lane);
        __syncthreads();                                     // R complete; every wave is done with this tile's halo image
        if (more) store_a();
        wino_store_Y<1>(Rs, p, img, oy0, (bx0 + t) * 16, 0, wa, lane);
        __syncthreads();                                     // next halo visible; Rs free again
    }
}

template <int CH>
static hipError_t launch_conv_wino_res_t(const ConvParams& p, hipStream_t s) {
    const int tiles_x = (p.out.w + 15) / 16, tiles_y = (p.out.h + 7) / 8;
    // tiles per workgroup: as many as keep >= ~2 workgroups per CU-slot in the launch
    int tpw = 16;
    while (tpw > 1 && (size_t)p.n * tiles_y * ((tiles_x + tpw - 1) / tpw) < 2048) tpw >>= 1;
    const int segs_x = (tiles_x + tpw - 1) / tpw;
    const size_t grid = (size_t)p.n * tiles_y * segs_x;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = (size_t)CH * 4 * 10 * 12 * 16 + (size_t)4 * 2 * 32 * 32 * 4;
    hipLaunchKernelGGL((conv_wino_res_kernel<CH>), dim3((unsigned)grid), dim3(256), lds, s, p, tiles_x, tiles_y, segs_x, tpw);
    return hipGetLastError();
}

int conv_wino_ntile(int cout) { return (cout % 64 == 0 || cout > 64) ? 64 : 32; }

hipError_t launch_conv_wino(const ConvParams& p, hipStream_t s) {
    if (p.resident && p.coutp == 32 && p.cin_chunks >= 1 && p.cin_chunks <= 4) {
        switch (p.cin_chunks) {
            case 1: return launch_conv_wino_res_t<1>(p, s);
            case 2: return launch_conv_wino_res_t<2>(p, s);
            case 3: return launch_conv_wino_res_t<3>(p, s);
            default: return launch_conv_wino_res_t<4>(p, s);
        }
    }
    return conv_wino_ntile(p.out.c) == 64 ? launch_conv_wino_t<2, 1>(p, s) : launch_conv_wino_t<1, 1>(p, s);
}

}  // namespace ecseg
