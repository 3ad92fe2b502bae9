// Filter transforms and re-layouts done once at model load: functions from host arrays to host arrays (the images the kernels
// stream), nothing of the handle and no device call.
#include "ctx.h"

namespace ecseg {

// Keras HWIO kernel -> wt[tap][chunk][half][NP][4] (zero padded; padded chunk / tap pitches, see common.h)
std::vector<float> relayout_conv(const float* w, int R, int S, int cin, int cout, int chunks, int np) {
    const size_t cp = (size_t)wt_chunk_pitch(np), tp = (size_t)wt_tap_pitch(np, chunks);
    std::vector<float> o((size_t)R * S * tp, 0.f);
    for (int t = 0; t < R * S; ++t)
        for (int ci = 0; ci < cin; ++ci) {
            const int chunk = ci / 8, hh = (ci % 8) / 4, e = ci % 4;
            const float* src = w + ((size_t)t * cin + ci) * cout;
            float* dst = o.data() + (size_t)t * tp + (size_t)chunk * cp + ((size_t)hh * np) * 4 + e;
            for (int co = 0; co < cout; ++co) dst[(size_t)co * 4] = src[co];
        }
    return o;
}
// Filter image of conv_wino16_kernel: MFMA A fragments [point 16][Cin / 16][Cout / 16][lane 64][k-step 4]; lane =
// (channel quad kq = lane / 16, output channel m = lane % 16) holds U[point][16 kc + 4 kq + s][16 nb + m] for s = 0..3
std::vector<float> relayout_wino16(const std::vector<float>& u, int cin, int cout) {
    const int KC = cin / 16, NB = cout / 16;
    std::vector<float> o((size_t)16 * KC * NB * 64 * 4);
    for (int pt = 0; pt < 16; ++pt)
        for (int kc = 0; kc < KC; ++kc)
            for (int nb = 0; nb < NB; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const int kq = lane >> 4, m = lane & 15;
                        o[((((size_t)pt * KC + kc) * NB + nb) * 64 + lane) * 4 + s] =
                            u[((size_t)pt * cin + 16 * kc + 4 * kq + s) * cout + 16 * nb + m];
                    }
    return o;
}
// Winograd F(2x2,3x3) filter transform U = G g G^T (float64), as 16 "taps" in HWIO order [a*4+b][cin][cout]
std::vector<float> winograd_filter(const float* w, int cin, int cout) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> u((size_t)16 * cin * cout);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co) {
            double g[3][3], t[4][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) g[r][c] = w[((size_t)(r * 3 + c) * cin + ci) * cout + co];
            for (int a = 0; a < 4; ++a)
                for (int c = 0; c < 3; ++c) t[a][c] = G[a][0] * g[0][c] + G[a][1] * g[1][c] + G[a][2] * g[2][c];
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b)
                    u[((size_t)(a * 4 + b) * cin + ci) * cout + co] =
                        (float)(t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2]);
        }
    return u;
}

// Winograd F(4x4,3x3) filter transform U = G g G^T (float64, 36 points) written straight in the per-wave stage layout
// of conv_wino4r_kernel and conv_wino4_kernel: wt4[cout block of 64][stage = 4 input channels][wave = half * 6 + xi][nu][h][cout 32][e], where
// stage s of 8-channel group s / 2 holds input channels 8 (s / 2) + 4 h + 2 (s % 2) + e.
std::vector<float> winograd4_filter(const float* w, int cin, int cout) {
    // G row of a finite point p: [1, p, p^2] / prod_{q != p} (p - q) over the finite points {0, +-a, +-b}; infinity: [0, 0, 1]
    // (textbook values for a = 1, b = 2: 1/4, -1/6, 1/24)
    const double a = W4_PA, b = W4_PB, a2 = a * a, b2 = b * b;
    const double n0 = a2 * b2, na = 2 * a2 * (a2 - b2), nb_ = 2 * b2 * (b2 - a2);
    const double G[6][3] = {{1 / n0, 0, 0},           {1 / na, a / na, a2 / na},   {1 / na, -a / na, a2 / na},
                            {1 / nb_, b / nb_, b2 / nb_}, {1 / nb_, -b / nb_, b2 / nb_}, {0, 0, 1}};
    // zero padded to whole 64-channel output blocks and whole 8-channel input groups (Cout % 64 == 32: the second
    // channel-half waves of the last block multiply zeros; Cin % 8 == 4: the second half of the last group is zero)
    const int nblk = (cout + 63) / 64, nstages = 2 * ((cin + 7) / 8);
    std::vector<float> o((size_t)nblk * nstages * 12 * 768, 0.f);
    for (int ci = 0; ci < cin; ++ci) {
        const int grp = ci / 8, r8 = ci % 8;
        const int hh = r8 / 4, ss = (r8 % 4) / 2, e = r8 % 2;
        const int stage = 2 * grp + ss;
        for (int co = 0; co < cout; ++co) {
            double g[3][3], t[6][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) g[r][c] = w[((size_t)(r * 3 + c) * cin + ci) * cout + co];
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 3; ++c) t[a][c] = G[a][0] * g[0][c] + G[a][1] * g[1][c] + G[a][2] * g[2][c];
            const int nb = co / 64, half = (co % 64) / 32, m = co % 32;
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) {
                    const double u = t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2];
                    // per (block, stage, wave): [point pair b / 2][lane = hh * 32 + m][point b % 2][channel e] - ONE ds_read_b128 per lane
                    // and point pair delivers the B operands of four MFMAs (round 4: three 16-byte reads per stage instead of six
                    // 8-byte ones; an LDS read beside the MFMA stream costs the matrix pipe ~14 cycles whatever its width)
                    const size_t idx = (((size_t)nb * nstages + stage) * 12 + (half * 6 + a)) * 768 + ((((size_t)(b >> 1) * 64 + hh * 32 + m) * 2 + (b & 1)) * 2) + e;
                    o[idx] = (float)u;
                }
        }
    }
    return o;
}

// Keras Conv2DTranspose kernel (kh, kw, out, in) -> one-tap GEMM filter over N = (a*kT + b) * coutp + co
std::vector<float> relayout_convt(const float* w, int kT, int cin, int cout, int chunks, int coutp) {
    const int np = kT * kT * coutp;
    const size_t cp = (size_t)wt_chunk_pitch(np), tp = (size_t)wt_tap_pitch(np, chunks);
    std::vector<float> o(tp, 0.f);
    for (int ab = 0; ab < kT * kT; ++ab)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) {
                const int chunk = ci / 8, hh = (ci % 8) / 4, e = ci % 4;
                o[(size_t)chunk * cp + ((size_t)hh * np + (size_t)ab * coutp + co) * 4 + e] = w[((size_t)ab * cout + co) * cin + ci];
            }
    return o;
}

// Keras Conv2DTranspose kernel (k, k, out, in), stride 2, k in {3, 4}, as the filter of a 2x2-tap convolution over the INPUT
// that produces all four output phases of a 2x2 output block at once: output (2 i + a, 2 j + b) of the full (uncropped)
// result sums w[a - 2 d][b - 2 e] x in(i + d, j + e) over d, e in {-1, 0} (taps with kernel index outside [0, k) are zero:
// 5 of 16 at k = 3, none at k = 4).  Layout as relayout_conv with tap t = (d + 1) * 2 + (e + 1) and N = (a * 2 + b) * coutp + co.
std::vector<float> relayout_convt_subpixel(const float* w, int k, int cin, int cout, int chunks, int coutp) {
    const int np = 4 * coutp;
    const size_t cp = (size_t)wt_chunk_pitch(np), tp = (size_t)wt_tap_pitch(np, chunks);
    std::vector<float> o((size_t)4 * tp, 0.f);
    for (int d = -1; d <= 0; ++d)
        for (int e = -1; e <= 0; ++e)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int kh = a - 2 * d, kw = b - 2 * e;
                    if (kh >= k || kw >= k) continue;
                    const int t = (d + 1) * 2 + (e + 1);
                    for (int co = 0; co < cout; ++co)
                        for (int ci = 0; ci < cin; ++ci) {
                            const int chunk = ci / 8, hh = (ci % 8) / 4, ee = ci % 4;
                            o[(size_t)t * tp + (size_t)chunk * cp + ((size_t)hh * np + (size_t)(a * 2 + b) * coutp + co) * 4 + ee] =
                                w[((size_t)(kh * k + kw) * cout + co) * cin + ci];
                        }
                }
    return o;
}

// Keras Conv2DTranspose kernel (k, k, out, in), stride 2, k in {3, 4}, PHASE BY PHASE (OpRt::ph_wt): output rows y = 2 j + c come from the
// kernel rows kh = c + crop (mod 2) at input offsets (c + crop - kh) / 2, so every output phase (c_y, c_x) is a forward convolution of
// 1 or 2 taps per axis over the input.  Returns, for phase c_y * 2 + c_x, its HWIO filter with the taps R x S and the leading pad.
std::array<PhaseFilter, 4> convt_phase_filters(const float* w, int k, int cin, int cout, int crop_top, int crop_left) {
    // taps of output phase c along one axis, ascending input offset: kernel index kh = c + crop (mod 2), offset (c + crop - kh) / 2
    auto taps = [&](int c, int crop, int idx[2], int& lead) {
        int n = 0, off[2] = {0, 0};
        for (int kk = k - 1; kk >= 0; --kk)
            if (((c + crop - kk) & 1) == 0) { off[n] = (c + crop - kk) / 2; idx[n] = kk; ++n; }      // kk descending = offset ascending
        lead = -off[0];
        return n;
    };
    std::array<PhaseFilter, 4> out;
    for (int cy = 0; cy < 2; ++cy)
        for (int cx = 0; cx < 2; ++cx) {
            PhaseFilter& f = out[cy * 2 + cx];
            int ky[2], kx[2];
            f.R = taps(cy, crop_top, ky, f.pt); f.S = taps(cx, crop_left, kx, f.pl);
            f.hwio.resize((size_t)f.R * f.S * cin * cout);
            for (int r = 0; r < f.R; ++r)
                for (int q = 0; q < f.S; ++q)
                    for (int ci = 0; ci < cin; ++ci)
                        for (int co = 0; co < cout; ++co)
                            f.hwio[(((size_t)r * f.S + q) * cin + ci) * cout + co] = w[(((size_t)ky[r] * k + kx[q]) * cout + co) * cin + ci];
        }
    return out;
}

}  // namespace ecseg
