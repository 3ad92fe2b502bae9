// The connected-component labelling engine for gfx950 (interface and what a pass leaves for its consumer: ccl.h): wavefront-level
// union-find on uint8 label images (n_img, H, W) and int32 parent arrays, and its direct users run_ccl_labels, run_count_cc and
// the test-only run_ccl_pass_debug.  HBM/latency-bound integer work; no MFMA.
//   * ccl_local: a workgroup labels one 64 x 32 tile in LDS.  One wavefront owns a 64-pixel row chunk; __ballot over
//     "run starts" gives every pixel the first pixel of its run without memory traffic or atomics; unions are issued
//     once per (run, upper-run) overlap instead of once per pixel pair - only the lane at the start of an overlap
//     calls unite(), the lock-free atomicMin union-find, so a root is the minimum raster index of its component;
//   * ccl_border: the same rule on the pixels along tile borders, on the global parent array;
//   * ccl_flatten: every pixel looks up its root; per-run (not per-pixel) atomics accumulate area / coordinate sums /
//     flag bits into the root's slot, per-wave popcounts accumulate component and pixel counts per key.
// blockIdx -> image mapping keeps all blocks of one image on one XCD (equal blockIdx % 8) so that the image's parent
// array stays in that XCD's L2.
#include "ccl.h"

namespace ecseg {

// union-find on the global parents: uf_load / uf_find / uf_unite, device_util.h (shared with fishdist_kernels.hip)

// ---- phase 1: label one 64 x 32 tile entirely in LDS ---------------------------------------------------------------
// Every workgroup labels its tile as if it were a stand-alone image: run heads by ballot, one LDS atomicMin union per
// (run, upper run) overlap, then every pixel's tile-local root is converted to a global pixel index and written out.
// Parent chains that phase 2 / ccl_flatten have to walk in global memory are thereby bounded by the number of tiles a
// component crosses, not by its height in pixels (a 1040-row background region used to cost ~1000 dependent loads).
__device__ __forceinline__ int lds_find(const volatile int* Ls, int x) {
    int n;
    while ((n = Ls[x]) != x) x = n;
    return x;
}
__device__ __forceinline__ void lds_unite(int* Ls, int a, int b) {
    for (;;) {
        a = lds_find(Ls, a);
        b = lds_find(Ls, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(Ls + a, b);
        if (old == a) return;
        a = old;
    }
}

// lane - 1 / lane + 1 of the whole wavefront in one VALU instruction (DPP wave shift; the end lane gets 0)
__device__ __forceinline__ int wave_from_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }   // wave_shr:1
__device__ __forceinline__ int wave_from_right(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }  // wave_shl:1

#ifndef ECSEG_CCL_WPE
#define ECSEG_CCL_WPE 8
#endif
template <int CONN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ECSEG_CCL_WPE, ECSEG_CCL_WPE))) void ccl_local_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                        int32_t* __restrict__ L_all, uint32_t* __restrict__ area_all,
                                                        u64* __restrict__ sumy_all, u64* __restrict__ sumx_all,
                                                        uint32_t* __restrict__ flag_all, int stat, int sparse,
                                                        uint8_t* __restrict__ tile_any, int allow_full,
                                                        int aux_mode, int aux_c, const uint8_t* __restrict__ aux_img, int need,
                                                        int32_t* __restrict__ G_all, uint32_t* __restrict__ own_bits) {
    __shared__ int Ls[CCL_BLOCK_ROWS * 64];
    __shared__ uint8_t Kl[4][64];                          // keys of every wave's last row (the next wave's "row above")
    // per-tile-component statistics (round 4: accumulated HERE, where a pixel's tile root is known from the LDS labelling, instead
    // of in a separate flatten pass that re-read every pixel's parent from global memory): bits 0-15 pixels of the slot
    // (<= 2048), bits 16-20 flag bits
    __shared__ uint32_t af_s[CCL_BLOCK_ROWS * 64];
    __shared__ int red[8];                                 // npx[1..3]
    extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
    // [TP] only when STAT_SUMS: coordinate sums of the slot RELATIVE to the tile origin, packed (sum of rows << 32 | sum of
    // columns; each < 2^18 inside a 64 x 32 tile): one 64-bit LDS atomic per run
    u64* sum_s = reinterpret_cast<u64*>(dyn_smem);
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;            // block-uniform
    const size_t base = (size_t)img * g.H * g.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool want_slots = stat != 0 || aux_mode != AUX_NONE;
    if (want_slots) {
        for (int i = threadIdx.x; i < CCL_BLOCK_ROWS * 64; i += 256) {
            af_s[i] = 0u;
            if (stat & STAT_SUMS) sum_s[i] = 0ull;
        }
    }
    if (threadIdx.x < 8) red[threadIdx.x] = 0;
    const int x = cx * 64 + lane;
    const int yblk = y0 - wave * CCL_ROWS;                 // first row of the tile
    // Empty-tile pre-pass (round 4): in the class labellings of a realistic image most tiles hold no keyed pixel at all, and the
    // vote below used to come after the whole first pass (8 byte loads, DPP shifts, ballots and LDS writes per thread).  For an
    // interior tile of an 8-byte-aligned image each thread now looks at 8 pixels with ONE 8-byte load first (lane = row lane / 8,
    // columns 8 (lane % 8) ...): no keyed pixel in the workgroup -> the tile is voted empty and left after ~30 instructions.
    if (sparse && !allow_full && (g.W & 7) == 0 && cx * 64 + 64 <= g.W && yblk + CCL_BLOCK_ROWS <= g.H &&
        (reinterpret_cast<uintptr_t>(img_all) & 7) == 0) {
        const u64 w8 = *reinterpret_cast<const u64*>(img_all + base + (size_t)(y0 + (lane >> 3)) * g.W + cx * 64 + (lane & 7) * 8);
        int anyk = 0;
        if (lut == LUT_NONZERO || lut == LUT_MULTI) anyk = w8 != 0ull;       // (labels are 0..3: key != 0 <=> value != 0)
        else {
#pragma unroll
            for (int b = 0; b < 8; ++b) anyk |= key_of((uint8_t)(w8 >> (8 * b)), lut);
        }
        if (!__syncthreads_or(anyk)) {
            if (threadIdx.x == 0) tile_any[tile_index(g, img)] = 0;
            return;
        }
    }
    // Full-tile pre-pass (round 5), the mirror image for the background labellings of fill_holes (allow_full: binary keys,
    // 4-connectivity, no statistics): most tiles of a realistic image hold no pixel of the class being filled at all - every
    // pixel is keyed and the tile is ONE node.  Decided from one 8-byte load per thread; such a tile used to run the whole
    // first pass (8 byte loads, DPP shifts, ballots and LDS writes per thread) before it found out.
    if (allow_full && (g.W & 7) == 0 && cx * 64 + 64 <= g.W && yblk + CCL_BLOCK_ROWS <= g.H &&
        (reinterpret_cast<uintptr_t>(img_all) & 7) == 0) {
        const u64 w8 = *reinterpret_cast<const u64*>(img_all + base + (size_t)(y0 + (lane >> 3)) * g.W + cx * 64 + (lane & 7) * 8);
        int unkeyed = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) unkeyed |= key_of((uint8_t)(w8 >> (8 * b)), lut) == 0;
        if (!__syncthreads_or(unkeyed)) {
            if (threadIdx.x == 0) {
                tile_any[tile_index(g, img)] = 2;
                const size_t p0 = base + (size_t)yblk * g.W + cx * 64;
                L_all[p0] = yblk * g.W + cx * 64;
                const bool edge = yblk == 0 || yblk + CCL_BLOCK_ROWS >= g.H || cx == 0 || cx * 64 + 64 >= g.W;
                flag_all[p0] = (aux_mode == AUX_BORDER && edge) ? 1u : 0u;
            }
            return;
        }
    }
    const u64 upto = (2ull << lane) - 1ull;                // lanes <= this one
    // The keys of the wave's 8 rows stay in registers: the neighbours above come from the previous row's register through
    // DPP wave shifts (one VALU instruction each) instead of byte reads from an LDS copy of the tile.
    // one packed word per row keeps the kernel at 8 waves per SIMD (four arrays of 8 registers each cost three of them and 40 %
    // of the kernel's speed): bits 0-1 key, 2-7 lane of the pixel's run head, 8-15 pixel value, 16-27 tile root + 1
    uint32_t info[CCL_ROWS];
#define KEY_OF(r) ((int)(info[r] & 3u))
#define HPOS_OF(r) ((int)((info[r] >> 2) & 63u))
#define VAL_OF(r) ((int)((info[r] >> 8) & 255u))
#define TROOT_OF(r) ((int)(info[r] >> 16) - 1)
    int hole = 0;                                          // a valid pixel of this thread without a key
    int rowmask = 0;                                       // (wave-uniform) bit r: row r of this wave holds a keyed pixel
    // all eight rows' bytes first (one round trip to memory instead of eight: the wave-uniform `continue` below keeps the compiler
    // from hoisting the later rows' loads itself - the whole kernel is a chain of latencies when a single image leaves each SIMD
    // with two or three waves)
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r;
        info[r] = (y < g.H && x < g.W) ? (uint32_t)img_all[base + (size_t)y * g.W + x] << 8 : 0u;
    }
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r, li = (wave * CCL_ROWS + r) * 64 + lane;
        const bool valid = y < g.H && x < g.W;
        const uint8_t v = (uint8_t)(info[r] >> 8);
        const int key = valid ? key_of(v, lut) : 0;
        hole |= (valid && key == 0) ? 1 : 0;
        // rows without a keyed pixel (most rows of a realistic class labelling, even inside a busy tile) are skipped by every
        // later phase on a wave-uniform test: no DPP shifts, ballots or LDS traffic for them (their Ls slots are never read)
        if (__ballot(key != 0) == 0ull) { info[r] = (uint32_t)v << 8; continue; }
        rowmask |= 1 << r;
        const int kprev = wave_from_left(key);
        const bool start = key != 0 && kprev != key;       // (lane 0: kprev = 0)
        const u64 S = __ballot(start);
        const int hp = 63 - __clzll(S & upto);             // (meaningless where key == 0)
        info[r] = (uint32_t)key | ((uint32_t)(hp & 63) << 2) | ((uint32_t)v << 8);
        Ls[li] = key ? (li - lane) + hp : -1;
    }
    Kl[wave][lane] = (uint8_t)KEY_OF(CCL_ROWS - 1);
    int mine = 0;
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) mine |= KEY_OF(r);
    // sparse mode (every consumer of this labelling looks at the key before it reads a parent): a tile without a keyed
    // pixel writes nothing, the others write only their keyed pixels - the parents of background pixels stay stale
    // The vote is also left in tile_any for the later kernels of this labelling: ccl_border, ccl_flatten and count_roots
    // skip a tile without a keyed pixel before they load anything of it.
    const int any = __syncthreads_or(mine);
    // FULL tiles (allow_full: binary keys, 4-connectivity, no statistics - the background labellings of fill_holes, where
    // most tiles of a realistic image hold nothing but background): every valid pixel is keyed, so the tile is ONE
    // component whose root is its first pixel.  Only that pixel gets a parent; ccl_border / ccl_flatten / apply_fill_tile
    // stand in the tile root for any pixel of such a tile (tile_any == 2).
    const int holes = allow_full ? __syncthreads_or(hole) : 1;
    const bool full = allow_full && any && !holes;
    if (threadIdx.x == 0) tile_any[tile_index(g, img)] = (uint8_t)(full ? 2 : (any != 0));
    uint32_t* ob = own_bits + tile_index(g, img) * 64;     // owner bits of this tile: bit (li & 31) of word li >> 5
    if (!any && sparse) return;                            // (later kernels skip the tile on tile_any == 0: its owner bits are never read)
    if (full) {
        // the whole tile is one component and its first pixel the only owner; its "touches the image border" bit is the tile's
        if (threadIdx.x == 0) {
            const size_t p0 = base + (size_t)yblk * g.W + cx * 64;
            L_all[p0] = yblk * g.W + cx * 64;
            const bool edge = yblk == 0 || yblk + CCL_BLOCK_ROWS >= g.H || cx == 0 || cx * 64 + 64 >= g.W;
            flag_all[p0] = (aux_mode == AUX_BORDER && edge) ? 1u : 0u;
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int ly = wave * CCL_ROWS + r, li = ly * 64 + lane;
        if (!((rowmask >> r) & 1)) continue;
        const int key = KEY_OF(r);
        const int above = r ? KEY_OF(r > 0 ? r - 1 : 0) : (wave ? (int)Kl[wave > 0 ? wave - 1 : 0][lane] : 0);
        const int al = wave_from_left(above), ar = wave_from_right(above), kl = wave_from_left(key);   // all lanes active here
        if (!key || ly == 0) continue;
        const bool left = kl == key, u0 = above == key, ul = al == key, ur = ar == key;
        if (CONN == 8) {
            if (ur && !u0) lds_unite(Ls, li, li - 63);
            if (!left) {
                if (u0) lds_unite(Ls, li, li - 64);
                else if (ul) lds_unite(Ls, li, li - 65);
            }
        } else {
            if (u0 && !(left && ul)) lds_unite(Ls, li, li - 64);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r, li = (wave * CCL_ROWS + r) * 64 + lane;
        if (!((rowmask >> r) & 1)) {
            if (!sparse && y < g.H && x < g.W) L_all[base + (size_t)y * g.W + x] = -1;
            continue;
        }
        const int key = KEY_OF(r);
        // run heads look the tile root up and leave it in their own slot (only finds run in this phase: a reader sees the
        // old parent or the root, both are on the chain); the rest of the run reads the head's slot - LDS operations of one
        // wave complete in order
        const bool head = key != 0 && HPOS_OF(r) == lane;
        if (head) {
            const int root = lds_find(Ls, li);
            Ls[li] = root;
        }
        const int rl = key ? Ls[(li - lane) + HPOS_OF(r)] : -1;
        info[r] |= (uint32_t)(rl + 1) << 16;                   // tile-local index of the pixel's tile root (+ 1; 0 = unkeyed)
        if (y < g.H && x < g.W) {
            const size_t p = base + (size_t)y * g.W + x;
            int lab = -1;
            if (key) lab = (yblk + (rl >> 6)) * g.W + cx * 64 + (rl & 63);
            if (key || !sparse) L_all[p] = lab;            // a pixel points at its TILE root for good; only tile roots are re-linked later
        }
    }
    // ---- per-run accumulation into the tile root's LDS slot (runs of equal key = runs of equal tile root) ----
    int npx[4] = {0, 0, 0, 0};
    if (want_slots || (need & NEED_NPX)) {
#pragma unroll
        for (int r = 0; r < CCL_ROWS; ++r) {
            const int y = y0 + r;
            const int key = KEY_OF(r), tr = TROOT_OF(r);
            if (need & NEED_NPX) {
#pragma unroll
                for (int k = 1; k < 4; ++k) npx[k] += __popcll(__ballot(key == k));
            }
            if (!want_slots || !((rowmask >> r) & 1)) continue;
            const u64 F = __ballot(key != 0);
            uint32_t bits = 0;
            if (aux_mode == AUX_BORDER) bits = (key && (y == 0 || y == g.H - 1 || x == 0 || x == g.W - 1)) ? 1u : 0u;
            else if (aux_mode == AUX_VALUE_EQ) bits = (key && VAL_OF(r) == aux_c) ? 1u : 0u;
            else if (aux_mode == AUX_IMAGE) bits = key ? aux_img[base + (size_t)y * g.W + x] : 0u;
            u64 B[5];
            const int nb = (aux_mode == AUX_IMAGE) ? 5 : (aux_mode == AUX_NONE ? 0 : 1);
#pragma unroll
            for (int b = 0; b < 5; ++b) B[b] = (b < nb) ? __ballot((bits >> b) & 1u) : 0ull;
            // a row without a flagged pixel has nothing to accumulate when only flags are wanted (fill_holes: rows off the image
            // border; merge_comp: rows without a class-c pixel) - wave-uniform
            if (!(stat & (STAT_AREA | STAT_SUMS)) && !(B[0] | B[1] | B[2] | B[3] | B[4])) continue;
            const bool start = key != 0 && HPOS_OF(r) == lane;
            const u64 S = __ballot(start);
            if (start) {
                const u64 above = ~((2ull << lane) - 1ull);
                const u64 stop = (S | ~F) & above;
                const int len = stop ? (__ffsll((long long)stop) - 1 - lane) : (64 - lane);
                const u64 run = (len == 64) ? ~0ull : (((1ull << len) - 1ull) << lane);
                if (stat & STAT_SUMS) {
                    const unsigned ry = (unsigned)(y - yblk), rx = (unsigned)lane, ulen = (unsigned)len;
                    atomicAdd(&sum_s[tr], ((u64)(ry * ulen) << 32) | (u64)(rx * ulen + ulen * (ulen - 1) / 2u));
                }
                uint32_t fb = 0;
#pragma unroll
                for (int b = 0; b < 5; ++b) if (B[b] & run) fb |= 1u << b;
                if (stat & (STAT_AREA | STAT_SUMS)) atomicAdd(&af_s[tr], (uint32_t)len);
                if (fb) atomicOr(&af_s[tr], fb << 16);
            }
        }
    }
    __syncthreads();
    // ---- owners (tile roots): partial statistics of the tile component into the owner's own global slots, owner bit for
    //      ccl_resolve (which walks only the owners and forwards their slots to the global roots) ----
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r, li = (wave * CCL_ROWS + r) * 64 + lane;
        if (!((rowmask >> r) & 1)) {
            if (lane == 0) { ob[2 * (wave * CCL_ROWS + r)] = 0u; ob[2 * (wave * CCL_ROWS + r) + 1] = 0u; }
            continue;
        }
        const bool own = KEY_OF(r) != 0 && TROOT_OF(r) == li;
        const u64 m = __ballot(own);
        if (lane == 0) { ob[2 * (wave * CCL_ROWS + r)] = (uint32_t)m; ob[2 * (wave * CCL_ROWS + r) + 1] = (uint32_t)(m >> 32); }
        if (own) {
            const size_t p = base + (size_t)y * g.W + x;
            const uint32_t af = want_slots ? af_s[li] : 0u;
            flag_all[p] = af >> 16;
            if (stat & STAT_AREA) area_all[p] = af & 0xffffu;
            if (stat & STAT_SUMS) {
                const u64 pk = sum_s[li], cnt = af & 0xffffu;
                sumy_all[p] = (pk >> 32) + (u64)yblk * cnt;
                sumx_all[p] = (pk & 0xffffffffull) + (u64)(cx * 64) * cnt;
            }
        }
    }
    if (need & NEED_NPX) {
        if (lane == 0) {
#pragma unroll
            for (int k = 1; k < 4; ++k) if (npx[k]) atomicAdd(&red[k], npx[k]);
        }
        __syncthreads();
        int32_t* G = g_shard(G_all, g, img);
        if (threadIdx.x >= 1 && threadIdx.x < 4 && red[threadIdx.x]) atomicAdd(G + G_NPX + threadIdx.x, red[threadIdx.x]);
    }
}
#undef KEY_OF
#undef HPOS_OF
#undef VAL_OF
#undef TROOT_OF

// ---- phase 2: unions across tile borders (global atomicMin union-find) ----------------------------------------------
// Workgroup = one tile, two waves: wave 0 takes the 64 pixels of the tile's first row (contacts with the tile above and,
// for its first pixel, with the tile to the left), wave 1 the 32 + 32 pixels of the first and last column of the other
// rows (lane = row | side << 5).  Every border pixel is one lane of ONE pass, so the dependent global loads of the
// union-find walks of a tile overlap instead of queueing row after row.
template <int CONN>
__global__ __launch_bounds__(128) void ccl_border_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                         int32_t* __restrict__ L_all, const uint8_t* __restrict__ tile_any) {
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const size_t ti = tile_index(g, img);
    const int ta = tile_any[ti];
    if (!ta) return;                                               // no keyed pixel in this tile: nothing to unite from here
    const size_t base = (size_t)img * g.H * g.W;
    const uint8_t* im = img_all + base;
    int32_t* L = L_all + base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ytile = y0 - wave * CCL_ROWS;                        // first row of the tile
    const int W = g.W;
    // full tiles (ccl_local, 4-connectivity only): only the tile's first pixel has a parent - it stands in for every pixel of
    // the tile; two full tiles are united once, by one lane
    const bool fullA = CONN == 4 && ta == 2;
    const int rootA = ytile * W + cx * 64;
    if (wave == 0) {
        // first row of a tile that has a tile above it
        const int y = ytile, x = cx * 64 + lane;
        if (y == 0 || x >= W) return;
        const int p = y * W + x;
        const int key = key_of(im[p], lut);
        if (!key) return;
        const bool left = x > 0 && key_of(im[p - 1], lut) == key;
        const bool fullL = CONN == 4 && lane == 0 && cx > 0 && tile_any[ti - 1] == 2;
        const bool fullU = CONN == 4 && tile_any[ti - g.chunks_x] == 2;
        const int P = fullA ? rootA : p;
        if (lane == 0 && left) uf_unite(L, P, fullL ? rootA - 64 : p - 1);
        const bool u0 = key_of(im[p - W], lut) == key;
        const bool ul = x > 0 && key_of(im[p - W - 1], lut) == key;
        const bool ur = x + 1 < W && key_of(im[p - W + 1], lut) == key;
        if (CONN == 8) {
            if (ur && !u0) uf_unite(L, p, p - W + 1);
            if (!left) {
                if (u0) uf_unite(L, p, p - W);
                else if (ul) uf_unite(L, p, p - W - 1);
            }
        } else {
            if (fullA && fullU) { if (lane == 0) uf_unite(L, rootA, rootA - CCL_BLOCK_ROWS * W); }
            else if (u0 && !(left && ul)) uf_unite(L, P, fullU ? rootA - CCL_BLOCK_ROWS * W : p - W);
        }
    } else {
        // first / last column of the rows that wave 0 does not cover (all rows of the image's first tile row)
        const int r = lane & 31, side = lane >> 5;
        const int y = ytile + r, x = cx * 64 + (side ? 63 : 0);
        if ((r == 0 && ytile > 0) || y >= g.H || x >= W) return;
        const int p = y * W + x;
        const int key = key_of(im[p], lut);
        if (!key) return;
        if (side == 0) {
            if (CONN == 4) {
                const bool fullL = cx > 0 && tile_any[ti - 1] == 2;
                if (x > 0 && key_of(im[p - 1], lut) == key) {
                    // two full tiles: one union is enough - the first row this wave handles (row 1, or row 0 in the top strip)
                    if (fullA && fullL) { if (r == (ytile > 0 ? 1 : 0)) uf_unite(L, rootA, rootA - 64); }
                    // one union per VERTICAL RUN of border contacts (round 4): when the pair above (p - W, p - W - 1) is a contact
                    // too, it is united by the lane above (or by wave 0 for the tile's first row) and both pixels hang on it
                    // vertically inside their own tiles - this union would walk two long chains of the background component
                    // to find them equal (32 such walks per tile edge were most of this kernel's time in the fill_holes labellings)
                    else if (r > 0 && key_of(im[p - W], lut) == key && key_of(im[p - W - 1], lut) == key) { }
                    else uf_unite(L, fullA ? rootA : p, fullL ? rootA - 64 : p - 1);
                }
                return;
            }
            if (x > 0 && key_of(im[p - 1], lut) == key) uf_unite(L, p, p - 1);
            if (CONN == 8 && y > 0 && x > 0 && key_of(im[p - W - 1], lut) == key) uf_unite(L, p, p - W - 1);
        } else if (CONN == 8) {                                    // diagonal contact across the vertical tile border
            if (y > 0 && x + 1 < W && key_of(im[p - W + 1], lut) == key) uf_unite(L, p, p - W + 1);
        }
    }
}
// ---- phase 3: resolve the tile roots ----------------------------------------------------------------------------------
// After ccl_local every pixel points at its tile root (the "owner" of a tile component) and the owner's global slots hold
// the component's statistics within the tile; ccl_border has linked owners across tiles.  Only the owners are touched
// here: each walks to its global root once, keeps it as its parent (a consumer reads a pixel's component as L[L[p]]: pixel
// -> owner -> global root) and forwards its slots to the root's with at most four global atomics.  No per-pixel pass: the
// int32 parent image is written once (ccl_local) and read once (the consumer).  (Rounds 1-3 re-read every pixel's parent
// here to rebuild the per-tile sums and rewrote it with the global root: ccl_flatten, 25 % of the post-processing time.)
// aux bits OR-ed into flag[root] (set per run by ccl_local): AUX_BORDER bit0 = touches the image border, AUX_VALUE_EQ
// bit0 = holds a pixel with value == aux_c, AUX_IMAGE bits of aux_img[p].
__global__ __launch_bounds__(256) void ccl_resolve_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                          int32_t* __restrict__ L_all, uint32_t* __restrict__ area_all,
                                                          u64* __restrict__ sumy_all, u64* __restrict__ sumx_all,
                                                          uint32_t* __restrict__ flag_all, int32_t* __restrict__ G_all,
                                                          int stat, int need,
                                                          int32_t* __restrict__ list1, int32_t* __restrict__ list2, size_t list_cap,
                                                          const uint8_t* __restrict__ tile_any, const uint32_t* __restrict__ own_bits) {
    constexpr int TP = CCL_BLOCK_ROWS * 64;                    // pixels per tile
    __shared__ int red[16];                                    // ncomp[1..3] at [0..2], last root [8], list counts [9..10], list bases [11..12], owners [13]
    __shared__ uint16_t own_s[TP];                             // compacted list of the owners
    __shared__ int16_t lsl_s[TP];                              // NEED_LISTS: (class << 12 | index inside the block's range) of owner k, -1 = none
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;                 // block-uniform
    const int tid = threadIdx.x;
    const size_t ti = tile_index(g, img);
    const int ta = tile_any[ti];
    if (!ta) return;                                           // ccl_local's vote: no keyed pixel, no owner
    const size_t base = (size_t)img * g.H * g.W;
    const uint8_t* im = img_all + base;
    int32_t* L = L_all + base;
    const int W = g.W;
    const int yblk = y0 - (tid >> 6) * CCL_ROWS;
    if (ta == 2) {
        // full tile (fill_holes background labelling: no statistics, no counters): its first pixel is the only owner
        if (tid == 0) {
            const int p0 = yblk * W + cx * 64;
            const int gr = uf_find(L, p0);
            if (gr != p0) {
                L[p0] = gr;
                const uint32_t f = flag_all[base + p0];
                if (f) atomicOr(flag_all + base + gr, f);
            }
        }
        return;
    }
    if (tid < 16) red[tid] = 0;
    __syncthreads();
    // owners -> compact list (thread = 8 consecutive pixels of the tile = one byte of the owner bits)
    {
        const uint32_t bits = (own_bits[ti * 64 + (tid >> 2)] >> ((tid & 3) * 8)) & 0xffu;
        if (bits) {
            int at = atomicAdd(&red[13], __popc(bits));
            uint32_t b = bits;
            while (b) {
                const int k = __ffs((int)b) - 1;
                b &= b - 1;
                own_s[at++] = (uint16_t)(tid * 8 + k);
            }
        }
    }
    __syncthreads();
    const int n_own = red[13];
    int32_t* G = g_shard(G_all, g, img);
    int ncomp[4] = {0, 0, 0, 0};
    int last_root = 0;
    // thread k takes owner k: the chain walks and global atomics of all owners of a tile are in flight together
    for (int k = tid; k < n_own; k += 256) {
        const int li = own_s[k];
        const int p = (yblk + (li >> 6)) * W + cx * 64 + (li & 63);
        const int gr = uf_find(L, p);
        int16_t ls = -1;
        if (gr != p) {
            L[p] = gr;                                         // (a concurrent walk through p sees the old parent or the root: both on the chain)
            if (stat & STAT_AREA) atomicAdd(area_all + base + gr, area_all[base + p]);
            if (stat & STAT_SUMS) {
                atomicAdd(sumy_all + base + gr, sumy_all[base + p]);
                atomicAdd(sumx_all + base + gr, sumx_all[base + p]);
            }
            const uint32_t f = flag_all[base + p];
            if (f) atomicOr(flag_all + base + gr, f);
        } else {                                               // a global root lives in this tile
            const uint8_t v = im[p];
            if (need & NEED_NCOMP) ncomp[key_of(v, lut) & 3] += 1;
            last_root = max(last_root, p + 1);
            // roots of class 1 / 2 go to the per-image lists (nucleus test)
            if ((need & NEED_LISTS) && (v == 1 || v == 2)) ls = (int16_t)((v << 12) | atomicAdd(&red[8 + v], 1));
        }
        if (need & NEED_LISTS) lsl_s[k] = ls;
    }
    if (!(need & (NEED_NCOMP | NEED_LAST | NEED_LISTS))) return;
    __syncthreads();
    if (need & NEED_LISTS) {
        // one global atomic per workgroup and class reserves the block's range in the image's list
        if (tid < 2 && red[9 + tid]) red[11 + tid] = atomicAdd(G_all + (size_t)img * G_IMG + (tid == 0 ? G_NLIST1 : G_NLIST2), red[9 + tid]);
        __syncthreads();
        for (int k = tid; k < n_own; k += 256) {
            const int ls = lsl_s[k];
            if (ls < 0) continue;
            const int v = ls >> 12, idx = ls & 0xfff, li = own_s[k];
            const int p = (yblk + (li >> 6)) * W + cx * 64 + (li & 63);
            if (v == 1) list1[(size_t)img * list_cap + red[11] + idx] = p;
            else list2[((size_t)img * list_cap + red[12] + idx) * 4] = p;      // first word of the chromosome's centroid slot
        }
    }
    // per-image counters: registers -> LDS -> one global atomic per workgroup and counter
    if (need & NEED_NCOMP) {
#pragma unroll
        for (int k = 1; k < 4; ++k) if (ncomp[k]) atomicAdd(&red[k - 1], ncomp[k]);
    }
    if ((need & NEED_LAST) && last_root) atomicMax(&red[8], last_root);
    __syncthreads();
    if (tid < 3) { if (red[tid]) atomicAdd(G + G_NCOMP + 1 + tid, red[tid]); }
    else if (tid == 8) { if (red[8]) atomicMax(G + G_LAST_ROOT, red[8]); }
}

// count_cc needs no resolve: after ccl_local + ccl_border a component's root is the one OWNER that still points at itself, so
// the components per key are counted from the owner bits (256 B per tile) and the owners' parents alone; the pixels per key were
// counted by ccl_local (NEED_NPX).  (Rounds 2-3 re-read image and parents of every pixel for this: 220 us per 64 speckled images.)
__global__ __launch_bounds__(256) void count_roots_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                          const int32_t* __restrict__ L_all, int32_t* __restrict__ G_all,
                                                          const uint8_t* __restrict__ tile_any, const uint32_t* __restrict__ own_bits) {
    __shared__ int red[4];
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const size_t ti = tile_index(g, img);
    const int tid = threadIdx.x;
    if (tile_any[ti]) {                                        // block-uniform
        if (tid < 4) red[tid] = 0;
        __syncthreads();
        const size_t base = (size_t)img * g.H * g.W;
        const int yblk = y0 - (tid >> 6) * CCL_ROWS;
        // (no pass combines allow_full with counting today, the full tile is handled all the same)
        uint32_t bits = thread_owner_bits(tile_any[ti], own_bits, ti, tid);
        int nc[4] = {0, 0, 0, 0};
        while (bits) {
            const int p = pop_owner(bits, g, tid, yblk, cx);
            if (L_all[base + p] == p) nc[key_of(img_all[base + p], lut) & 3] += 1;
        }
#pragma unroll
        for (int k = 1; k < 4; ++k) if (nc[k]) atomicAdd(&red[k], nc[k]);
        __syncthreads();
        int32_t* G = g_shard(G_all, g, img);
        if (tid >= 1 && tid < 4 && red[tid]) atomicAdd(G + G_NCOMP + tid, red[tid]);
    }
}

// fold the G_SHARDS replicas of every image's counter block into replica 0
__global__ void reduce_g_kernel(int32_t* __restrict__ G_all, int n_img) {
    const int im = blockIdx.x, t = threadIdx.x;          // blockDim = G_STRIDE
    if (im >= n_img) return;
    int32_t* G = G_all + (size_t)im * G_IMG;
    int v = G[t];
    for (int sh = 1; sh < G_SHARDS; ++sh) {
        const int w = G[sh * G_STRIDE + t];
        v = (t == G_LAST_ROOT) ? max(v, w) : v + w;
        G[sh * G_STRIDE + t] = 0;                         // folded: a second fold (count_flagged_owner_roots adds later) adds nothing twice
    }
    G[t] = v;
}

__global__ void zero_g_kernel(int32_t* G, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) G[i] = 0;
}
void launch_zero_g(int32_t* G, int n, hipStream_t s) {
    hipLaunchKernelGGL(zero_g_kernel, dim3((n + 255) / 256), dim3(256), 0, s, G, n);
}

hipError_t run_ccl_pass(PostWorkspace& ws, const CclGeom& g, const CclPass& c, hipStream_t s) {
    int32_t* const G = c.g ? c.g : ws.g;
    // (a pass that produces no counters - the fill_holes labellings - touches none: no zeroing launch)
    if (c.need && !c.g) launch_zero_g(G, g.n_img * G_IMG, s);
    const unsigned grid = geom_grid(g);
    const bool slots = !c.count_only;                          // count_only: counts per key only - no statistics, no owners' slots
    const int stat = slots ? c.stat : 0, aux_mode = slots ? c.aux_mode : AUX_NONE;
    const int need_local = c.need & NEED_NPX;                  // pixels per key: counted where the keys are in registers
    const size_t dyn = (stat & STAT_SUMS) ? (size_t)CCL_BLOCK_ROWS * 64 * 8 : 0;
    if (c.conn == 8) {
        hipLaunchKernelGGL(ccl_local_kernel<8>, dim3(grid), dim3(256), dyn, s, g, c.key_img, c.lut, ws.L, ws.area, ws.sumy,
                           ws.sumx, ws.flag, stat, c.sparse ? 1 : 0, ws.tile_any, 0, aux_mode, c.aux_c, c.aux_img, need_local,
                           G, ws.own_bits);
        hipLaunchKernelGGL(ccl_border_kernel<8>, dim3(grid), dim3(128), 0, s, g, c.key_img, c.lut, ws.L, ws.tile_any);
    } else {
        hipLaunchKernelGGL(ccl_local_kernel<4>, dim3(grid), dim3(256), dyn, s, g, c.key_img, c.lut, ws.L, ws.area, ws.sumy,
                           ws.sumx, ws.flag, stat, c.sparse ? 1 : 0, ws.tile_any,
                           (c.allow_full && c.stat == 0 && c.need == 0 && !c.count_only) ? 1 : 0, aux_mode, c.aux_c, c.aux_img,
                           need_local, G, ws.own_bits);
        hipLaunchKernelGGL(ccl_border_kernel<4>, dim3(grid), dim3(128), 0, s, g, c.key_img, c.lut, ws.L, ws.tile_any);
    }
    if (c.count_only) {        // counts per key only: no per-pixel roots, no statistics
        hipLaunchKernelGGL(count_roots_kernel, dim3(grid), dim3(256), 0, s, g, c.key_img, c.lut, ws.L, G, ws.tile_any, ws.own_bits);
        if (!c.g) hipLaunchKernelGGL(reduce_g_kernel, dim3(g.n_img), dim3(G_STRIDE), 0, s, G, g.n_img);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(ccl_resolve_kernel, dim3(grid), dim3(256), 0, s, g, c.key_img, c.lut, ws.L, ws.area, ws.sumy, ws.sumx,
                       ws.flag, G, c.stat, c.need, c.list1, c.list2, c.list_cap, ws.tile_any, ws.own_bits);
    if (c.need && !c.g) hipLaunchKernelGGL(reduce_g_kernel, dim3(g.n_img), dim3(G_STRIDE), 0, s, G, g.n_img);
    return hipGetLastError();
}

// fold != 0: the pass had a counter block of its own whose replicas nobody has folded yet
__global__ void gather_counts_kernel(const int32_t* __restrict__ G_all, int n_img, int key, int32_t* __restrict__ n_out,
                                     long long* __restrict__ px_out, long long full_px, int fold) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const int32_t* G = G_all + (size_t)i * G_IMG;
    const int n = fold ? g_fold_sum(G, G_NCOMP + key) : G[G_NCOMP + key];
    const long long px = fold ? g_fold_sum(G, G_NPX + key) : G[G_NPX + key];
    if (n_out) n_out[i] = n;
    // count_cc's pixel total (src/image_tools.py:116-119) is float 0.0 when nothing is counted: no component, or no
    // background label for np.unique(...)[1:] to drop (mask without a single zero pixel)
    if (px_out) px_out[i] = (n == 0 || px == full_px) ? -1 : px;
}
void launch_gather_counts(const int32_t* G_all, int n_img, int key, int32_t* n_out, long long* px_out, long long full_px, int fold, hipStream_t s) {
    hipLaunchKernelGGL(gather_counts_kernel, dim3((n_img + 63) / 64), dim3(64), 0, s, G_all, n_img, key, n_out, px_out, full_px, fold);
}

// ---- the direct users of a pass: count_cc, labels, flag queries, and the test-only export -----------------------------------
hipError_t run_count_cc(PostWorkspace& ws, const uint8_t* mask, int n_img, int H, int W, int32_t* n_dev, long long* px_dev,
                        hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    const CclGeom g = make_geom(n_img, H, W);
    CclPass p{mask, LUT_NONZERO, 8, 0, AUX_NONE, 0, nullptr, NEED_NCOMP | NEED_NPX, true};
    p.sparse = true;                                           // count_roots looks at the key first
    hipError_t e = run_ccl_pass(ws, g, p, s);
    if (e != hipSuccess) return e;
    launch_gather_counts(ws.g, n_img, 1, n_dev, px_dev, (long long)H * W, 0, s);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void export_labels_kernel(const int32_t* __restrict__ L, int32_t* __restrict__ out, size_t total, size_t px) {
    PX_LOOP(total) {                    // background -1 -> 0, component -> 1 + raster index of its first pixel (pixel -> owner -> global root)
        const int o = L[t];
        out[t] = o < 0 ? 0 : L[(t / px) * px + o] + 1;
    }
}

hipError_t run_ccl_labels(PostWorkspace& ws, const uint8_t* mask, int n_img, int H, int W, int conn, int32_t* labels_dev,
                          hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    const CclGeom g = make_geom(n_img, H, W);
    CclPass p{mask, LUT_NONZERO, conn, 0, AUX_NONE, 0, nullptr, 0};
    hipError_t e = run_ccl_pass(ws, g, p, s);
    if (e != hipSuccess) return e;
    const size_t total = (size_t)n_img * H * W;
    hipLaunchKernelGGL(export_labels_kernel, dim3(px_grid(total)), dim3(256), 0, s, ws.L, labels_dev, total, (size_t)H * W);
    return hipGetLastError();
}

// Up to 5 counts of roots by (key, flag bits) in ONE pass over the owner bits (round 4): roots are owners that still point at
// themselves, so only the 256 B of owner bits per tile and the owners' parents / flags are read - the per-pixel scan below
// (image + parent of every pixel, once per query) took 6 x 181 us of the 3.9 ms overlay row of 64 images.
// The queries: FlagQueries, ccl.h (the counts land sharded: launch_flagged_counts folds them with reduce_g_kernel).
__global__ __launch_bounds__(256) void count_flagged_owner_roots_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                                        const int32_t* __restrict__ L_all,
                                                                        const uint32_t* __restrict__ flag_all,
                                                                        int32_t* __restrict__ G_all,
                                                                        const uint8_t* __restrict__ tile_any,
                                                                        const uint32_t* __restrict__ own_bits, FlagQueries Q) {
    __shared__ int red[8];
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const size_t ti = tile_index(g, img);
    const int ta = tile_any[ti];
    if (!ta) return;
    const int tid = threadIdx.x;
    if (tid < 8) red[tid] = 0;
    __syncthreads();
    const size_t base = (size_t)img * g.H * g.W;
    const int yblk = y0 - (tid >> 6) * CCL_ROWS;
    uint32_t bits = thread_owner_bits(ta, own_bits, ti, tid);
    int c[5] = {0, 0, 0, 0, 0};
    while (bits) {
        const int p = pop_owner(bits, g, tid, yblk, cx);
        if (L_all[base + p] != p) continue;
        const int key = key_of(img_all[base + p], lut);
        const uint32_t f = flag_all[base + p];
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (i < Q.n && (!Q.key[i] || key == Q.key[i]) && (f & Q.need[i]) == Q.need[i]) c[i] += 1;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) if (c[i]) atomicAdd(&red[i], c[i]);
    __syncthreads();
    int32_t* G = g_shard(G_all, g, img);
    if (tid < Q.n && red[tid]) atomicAdd(G + G_CNT0 + Q.slot[tid], red[tid]);
}

void launch_flagged_counts(PostWorkspace& ws, const CclGeom& g, const uint8_t* key_img, uint32_t lut, const FlagQueries& Q, hipStream_t s) {
    hipLaunchKernelGGL(count_flagged_owner_roots_kernel, dim3(geom_grid(g)), dim3(256), 0, s, g, key_img, lut, ws.L, ws.flag, ws.g,
                       ws.tile_any, ws.own_bits, Q);
    hipLaunchKernelGGL(reduce_g_kernel, dim3(g.n_img), dim3(G_STRIDE), 0, s, ws.g, g.n_img);
}

// ---- test-only: one pass alone, everything it produced read back (run_ccl_pass_debug) --------------------------------------
// One thread per pixel.  A keyed pixel's root is read as every consumer reads it: pixel -> owner -> root; in a full tile
// (tile_any == 2) the tile's first pixel stands in for the owner (apply_fill_tile_kernel).  The key comes first: a sparse pass
// leaves stale parents on background.  Root pixels carry their slots, every other pixel 0.  A count_only pass has no resolved
// roots: the pixels count_roots_kernel counts (owners that point at themselves) are exported as their own roots, the rest as -1.
__global__ __launch_bounds__(256) void export_pass_px_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint32_t lut,
                                                             const int32_t* __restrict__ L_all, const uint32_t* __restrict__ area_all,
                                                             const u64* __restrict__ sumy_all, const u64* __restrict__ sumx_all,
                                                             const uint32_t* __restrict__ flag_all, const uint8_t* __restrict__ tile_any,
                                                             const uint32_t* __restrict__ own_bits, int stat, int count_only,
                                                             int32_t* __restrict__ root_out, uint32_t* __restrict__ area_out,
                                                             u64* __restrict__ sumy_out, u64* __restrict__ sumx_out,
                                                             uint32_t* __restrict__ flag_out) {
    const size_t px = (size_t)g.H * g.W;
    IMG_PX_LOOP(g.n_img, px) {
        const int p = (int)(t - ib), y = p / g.W, x = p % g.W;
        const int ty = y / CCL_BLOCK_ROWS, tx = x / 64;
        const size_t ti = (size_t)im * g.blocks_per_img + (size_t)ty * g.chunks_x + tx;
        const int ta = tile_any[ti];
        const int p0 = ty * CCL_BLOCK_ROWS * g.W + tx * 64;            // the tile's first pixel
        int root = -1;
        uint32_t a = 0, f = 0;
        u64 sy = 0, sx = 0;
        if (key_of(img_all[t], lut)) {
            if (count_only) {
                const int li = (y - ty * CCL_BLOCK_ROWS) * 64 + (x - tx * 64);
                const bool owner = ta == 2 ? p == p0 : ((own_bits[ti * 64 + (li >> 5)] >> (li & 31)) & 1u) != 0;
                if (owner && L_all[t] == p) root = p;
            } else {
                const int o = ta == 2 ? p0 : L_all[t];
                root = (o >= 0 && (size_t)o < px) ? L_all[ib + o] : -2;
                if (root < 0 || (size_t)root >= px) root = -2;
                if (root == p) {
                    f = flag_all[t];
                    if (stat & STAT_AREA) a = area_all[t];
                    if (stat & STAT_SUMS) { sy = sumy_all[t]; sx = sumx_all[t]; }
                }
            }
        }
        root_out[t] = root; area_out[t] = a; sumy_out[t] = sy; sumx_out[t] = sx; flag_out[t] = f;
    }
}

// one thread per image: the folded counters (replica 0 after reduce_g_kernel)
__global__ void export_pass_counters_kernel(const int32_t* __restrict__ G_all, int n_img, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const int32_t* G = G_all + (size_t)i * G_IMG;
    int32_t* o = out + (size_t)i * CCL_DEBUG_COUNTERS;
    for (int k = 0; k < 3; ++k) { o[k] = G[G_NCOMP + 1 + k]; o[3 + k] = G[G_NPX + 1 + k]; }
    o[6] = G[G_LAST_ROOT]; o[7] = G[G_NLIST1]; o[8] = G[G_NLIST2];
    for (int k = 0; k < 5; ++k) o[9 + k] = G[G_CNT0 + k];
    o[14] = 0; o[15] = 0;
}

// one thread per list entry: the class-1 roots and the first word of every class-2 slot up to their counts, -1 beyond
__global__ __launch_bounds__(256) void export_pass_lists_kernel(const int32_t* __restrict__ G_all, const int32_t* __restrict__ list1,
                                                                const int32_t* __restrict__ list2, int n_img, size_t cap,
                                                                int32_t* __restrict__ out1, int32_t* __restrict__ out2) {
    IMG_PX_LOOP(n_img, cap) {
        const int k = (int)(t - ib);
        const int32_t* G = G_all + (size_t)im * G_IMG;
        out1[t] = (list1 && k < G[G_NLIST1]) ? list1[t] : -1;
        out2[t] = (list2 && k < G[G_NLIST2]) ? list2[t * 4] : -1;
    }
}

hipError_t run_ccl_pass_debug(PostWorkspace& ws, const uint8_t* key_img, const uint8_t* aux_img, int n_img, int H, int W,
                              const CclPassDesc& d, const CclPassExport& out, hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    // (ecseg_ccl_pass_debug says which: ECSEG_E_INVALID; see struct CclPass for the last two)
    if ((d.conn != 4 && d.conn != 8) || (d.aux_mode == AUX_IMAGE && !aux_img) || d.n_q < 0 || d.n_q > 5 ||
        ((d.need & NEED_LISTS) && d.conn != 8) || (d.n_q > 0 && d.count_only))
        return hipErrorInvalidValue;
    const CclGeom g = make_geom(n_img, H, W);
    const size_t px = (size_t)H * W, cap = ccl_list_cap(H, W);
    CclPass p{key_img, d.lut, d.conn, d.stat, d.aux_mode, d.aux_c, aux_img, d.need, d.count_only};
    p.sparse = d.sparse;
    p.allow_full = d.allow_full;
    if (d.need & NEED_LISTS) {                                 // carved as run_meta_inference carves them
        p.list1 = ws.list;
        p.list2 = reinterpret_cast<int32_t*>(reinterpret_cast<double2*>(ws.list + (((size_t)n_img * cap + 3) & ~(size_t)3)));
        p.list_cap = cap;
    }
    // a pass without counters zeroes none: the export and the flag queries below read them all the same
    if (!d.need) launch_zero_g(ws.g, n_img * G_IMG, s);
    hipError_t e = run_ccl_pass(ws, g, p, s);
    if (e != hipSuccess) return e;
    if (d.n_q > 0) {
        FlagQueries Q{d.n_q, {}, {}, {}};
        for (int k = 0; k < d.n_q; ++k) { Q.key[k] = d.q_key[k]; Q.need[k] = d.q_need[k]; Q.slot[k] = k; }
        launch_flagged_counts(ws, g, key_img, d.lut, Q, s);
    }
    hipLaunchKernelGGL(export_pass_px_kernel, img_grid(px, n_img), dim3(256), 0, s, g, key_img, d.lut, ws.L, ws.area, ws.sumy, ws.sumx,
                       ws.flag, ws.tile_any, ws.own_bits, d.stat, d.count_only ? 1 : 0, out.root, out.area, out.sumy, out.sumx, out.flag);
    hipLaunchKernelGGL(export_pass_counters_kernel, dim3((n_img + 63) / 64), dim3(64), 0, s, ws.g, n_img, out.counters);
    hipLaunchKernelGGL(export_pass_lists_kernel, img_grid(cap, n_img), dim3(256), 0, s, ws.g, p.list1, p.list2, n_img, cap, out.list1,
                       out.list2);
    return hipGetLastError();
}

}  // namespace ecseg
