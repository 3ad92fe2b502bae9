// Where the F(4x4) kernels (wino4_kernel.hip, wino4r_kernel.hip, wino4s_kernel.hip, wino4_combine.inc, wino4_head.inc) park their
// values in LDS: every lane -> address function of the three kernels in one place, as host + device constexpr code, so that the
// SAME functions the kernels call are walked by the host-side bank model (tools/lds_bank_model.cpp, tests/test_wino4_lds_banks.py),
// which applies the per-instruction bank rule of the LDS to every access site and reports the extra cycles.  The kernels hold no
// address arithmetic of their own: which lane computes what is theirs, where it lives is decided here.
//
// Units: a SLOT is 16 bytes (four channels of a pixel), an "8" suffix means units of 8 bytes (a channel pair), exchange-image
// indices are floats.  LDS map of a workgroup (slots from the start of the dynamic segment):
//   conv_wino4r / conv_wino4s:  [2][HS] raw halo | [TS] t image | 12 waves x 2 filter stages
//   conv_wino4 (split-K):       [3][HS] raw halo ring | 12 waves x 2 x [BWS] filter stages
//   output stage (all three):   24 planes x [RPLANE] floats of the exchange image, from slot 0 on, over whatever the K loop left
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define W4L_HD __host__ __device__ __forceinline__
#else
#define W4L_HD inline
#endif

// The region rule of the A-operand lane -> tile map (wino4_lane_tile.inc).  ds_read_b128 serves lanes {0-3,12-15,20-27} and {4-11,16-19,28-31} of
// each wave half in separate LDS cycles; each of those groups gets the 16 tiles of ONE region: lane quad q8 = (lane & 31) >> 2 belongs to region
// 0, 1, 1, 0, 1, 0, 0, 1.  The output stage applies the same rule to its tile-row pairs (two per tile row of the 32 tiles).  (A macro: as a
// function the rule compiles to other device code in the output stages of conv_wino4_kernel and conv_wino4r_kernel, EXPERIMENTS.md round 11.)
#define W4_QUAD_REGION(q8) ((0x96 >> (q8)) & 1)

namespace ecseg {

struct W4Lds {
    // ---- sizes ----
    static constexpr int HS = 1536;            // halo slots per raw buffer, 24 x 64 (one LDS-DMA piece = 64 slots): 1338 of them belong to the raw image of conv_wino4r / conv_wino4s, 1296 to the ring of conv_wino4
    // Raw image of conv_wino4r / conv_wino4s: 18 columns x 2 channel halves + ONE pad slot per row.  row_pass reads it in item order (8 contiguous bytes per
    // lane, 72 items per raw row, the next item group four raw rows on): with an even row the second run of a 16-lane group that straddles two
    // groups starts on the bank the first began on (4 rows x 36 slots = 0 mod 32 banks); 37 = 1 (mod 4) puts it on the bank the first run ends on,
    // for the 16-lane groups of an 8-byte pair read and for the 32-lane groups of a single one (REGION = 0 mod 16 for those)
    static constexpr int RAW_COLS = 36;        // slots of a raw row that hold a pixel
    static constexpr int RAW_ROW = 37;         // slots per raw row
    static constexpr int RAW_REGION = 672;     // slots per region: 18 x 37 = 666, padded
    static constexpr int RAW_USED = RAW_REGION + 18 * RAW_ROW;    // (the LDS-DMA fills pad slots and the rest of the buffer with zeros)
    // t image: slot(region, xi, tile row ty, half h, column x) = (region * 6 + xi) * T_BLOCK + t_row(ty) + h * T_HALF + t_pos(x).
    //   readers (load_t, 16-byte reads, 16 slots = 64 banks per lane group of one region): a group's 16 lanes are (ty, tx) = 4 x 4 tiles at
    //   t_row(ty) + 2 tx + const: t_row = {0, 9, 8, 1} (mod 16) + {0, 2, 4, 6} are 16 different slots of the bank row;
    //   writers (row_pass, 8-byte writes, 8 slots = 32 banks per 16 contiguous lanes = 4 consecutive columns x 2 halves x 2 channel pairs): columns
    //   4 m .. 4 m + 3 and 4 m + 2 .. 4 m + 5 land on t_pos = {0, 2, 1, 3} + 2 m and {1, 3, 2, 4} + 2 m (mod 8), the other half 20 = 4 (mod 8) slots on,
    //   and the group that runs from columns 16, 17 of an even tile row into columns 0, 1 of the next finds that row an odd number of slots on.
    //   (Until round 9: columns one slot apart, halves 18 and rows 36 slots apart - every write group met another on two of its eight slots.)
    static constexpr int T_HALF = 20;          // slots between the two channel halves of a column
    static constexpr int T_BLOCK = 168;        // slots per (region, transform row): t_row(3) + 39
    static constexpr int TS = 2 * 6 * T_BLOCK; // 2 regions x 6 transform rows
    static constexpr int BWS = 192;            // filter slots per wave and stage of the fp32 kernels: 6 points x 2 halves x 32 couts x 2 k / 4
    static constexpr int RPLANE = 1056;        // floats per (xi, x) plane of the output exchange image: 32 tiles x 32 couts + 32
    static constexpr int EPI_FLOATS = 24 * RPLANE;

    // ---- regrouped rows / columns of the split-K kernel's ring: 0..17 -> position; those of one phase modulo the tile stride 4 next to each other ----
    static W4L_HD constexpr int pos(int v) { return ((v & 3) == 0 ? 0 : (v & 3) == 1 ? 5 : (v & 3) == 2 ? 10 : 14) + (v >> 2); }
    static W4L_HD constexpr int inv(int r) { return r < 5 ? 4 * r : r < 10 ? 4 * (r - 5) + 1 : r < 14 ? 4 * (r - 10) + 2 : 4 * (r - 14) + 3; }

    // ---- raw halo image of conv_wino4r / conv_wino4s (only row_pass reads it; the LDS-DMA writes slot 64 piece + lane) ----
    // strides of the image, for the decode of an LDS-DMA slot in wino4_region.inc: slot = REGION * region + ROW * row + cc, cc = 2 column + channel half
    struct Raw { static constexpr int USED = RAW_USED, REGION = RAW_REGION, ROW = RAW_ROW, COLS = RAW_COLS; };     // (cc >= COLS: a pad slot)
    // row_pass read (the lane takes channel pair cpair = 8 bytes of the slot): raw row 4 tyy (+ i: + i * raw_row()) of region tgg, column x, half h
    static W4L_HD constexpr int raw_read(int buf, int tgg, int tyy, int x, int h) { return buf * HS + tgg * RAW_REGION + 4 * tyy * RAW_ROW + 2 * x + h; }
    static W4L_HD constexpr int raw_row() { return RAW_ROW; }

    // ---- t image (row-transformed halo of one group), slots from its start ----
    static W4L_HD constexpr int t_pos(int x) { return ((x & 3) == 0 ? 0 : (x & 3) == 1 ? 10 : (x & 3) == 2 ? 1 : 11) + 2 * (x >> 2); }    // column 0..17 -> 0..18
    static W4L_HD constexpr int t_row(int ty) { return 44 * ty - 3 * (ty & 1); }                                                        // tile row -> 0, 41, 88, 129
    // row_pass write (8 bytes of the slot: channel pair cpair) of transform row 0 (+ xi: + xi * t_xi())
    static W4L_HD constexpr int t_write(int tgg, int tyy, int h, int x) { return (tgg * 6) * T_BLOCK + t_row(tyy) + h * T_HALF + t_pos(x); }
    static W4L_HD constexpr int t_xi() { return T_BLOCK; }
    // load_t: the lane's tile (region tg, tile row ty, tile column tx, half lh of the wave) + the column j of its six
    static W4L_HD constexpr int t_lane(int tg, int xi, int ty, int lh, int tx) { return (tg * 6 + xi) * T_BLOCK + t_row(ty) + lh * T_HALF + t_pos(4 * tx); }
    static W4L_HD constexpr int t_col(int j) { return t_pos(j); }                 // (t_pos(4 tx + j) = t_pos(4 tx) + t_pos(j))

    // ---- raw halo ring of conv_wino4 (split-K): rows AND columns regrouped, the channel halves 18 slots apart ----
    struct Ring { static constexpr int USED = 2 * 18 * 36, REGION = 18 * 36, ROW = 36, COLS = 36; };      // slot = REGION * region + ROW * regrouped row + position in the row
    static W4L_HD constexpr int a_lane(int tg, int ty, int lh, int tx) { return (tg * 18 + ty) * 36 + lh * 18 + tx; }
    static W4L_HD constexpr int a_row(int r) { return 36 * pos(r); }
    static W4L_HD constexpr int a_col(int j) { return pos(j); }

    // ---- per-wave filter stages ----
    static W4L_HD constexpr int bw_stage(int wave, int buf) { return (wave * 2 + buf) * BWS; }                // fp32 kernels: slots from the first stage
    static W4L_HD constexpr int bw_read(int lane, int k) { return lane + k * 64; }                            // 16-byte read k (point pair k) of a stage
    static constexpr int S_STAGE = 3072;                                                                      // conv_wino4s: bytes per stage
    static W4L_HD constexpr int s_stage(int wave, int buf) { return (wave * 2 + buf) * S_STAGE; }             // bytes from the first stage
    static W4L_HD constexpr int s_read16(int lane, int cb) { return cb * 1024 + lane * 16; }                  // [u2|u1] of column block cb, bytes within the stage
    static W4L_HD constexpr int s_read8(int lane, int cb) { return 2048 + cb * 512 + lane * 8; }              // u3 of column block cb

    // ---- output exchange image, floats: plane (xi, x) = 4 xi + x ----
    static W4L_HD constexpr int r_plane(int n) { return n * RPLANE; }
    // fold write of plane (xi, 0) (+ x: + r_plane(x)): [32 tiles][32 couts] planes (fused head, conv_wino4s, conv_wino4)
    static W4L_HD constexpr int r_fold(int xi, int tl, int li) { return (xi * 4) * RPLANE + tl * 32 + li; }
    // the same in the tile-half form of conv_wino4r: [16 tiles][64 couts] planes
    static W4L_HD constexpr int r_fold_tile(int xi, int tl, int ch, int li) { return (xi * 4) * RPLANE + tl * 64 + ch * 32 + li; }
    // combine read of transform row 0 (+ k: + r_plane(4 k)): column cx of tile pair nw, tile nlo of the pair, channel quad cq
    static W4L_HD constexpr int r_comb(int cx, int nlo, int cq, int nw) { return cx * RPLANE + nlo * 32 + 4 * cq + nw * 64; }
    static W4L_HD constexpr int r_comb_tile(int cx, int nlo, int cq, int tp, int chh) { return cx * RPLANE + nlo * 64 + 4 * cq + tp * 128 + chh * 32; }
};

}  // namespace ecseg
