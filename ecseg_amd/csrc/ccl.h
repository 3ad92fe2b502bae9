// The connected-component labelling engine of the post-processing (ccl_kernels.hip) as its consumers see it.  Included by the post
// sources only: ccl_kernels.hip, meta_inference_kernels.hip, overlay_kernels.hip, stitch_preprocess_kernels.hip.
//
// What a consumer may read after run_ccl_pass (reference: skimage.measure.label / scipy.ndimage.label, src/image_tools.py:26,42-50,66-67,115):
//   * a pixel's "key" is a small integer derived from its value through a 4-entry LUT (0 = background); two neighbouring pixels are
//     connected iff their keys are equal and non-zero, so the disjoint class masks (img==1, img==2, img==3) are labelled in ONE pass;
//   * ws.L: after ccl_local every pixel points at its tile root (the "owner" of a tile component) for good; ccl_resolve leaves the
//     global root in the owner's parent, so a consumer reads a pixel's component as L[L[p]]: pixel -> owner -> global root.  The root
//     of a component is its first pixel in raster order (the order scipy/skimage number components in, which merge_comp's skipped
//     last component depends on, src/image_tools.py:27).  Unkeyed pixels hold -1, unless the pass is `sparse` (every consumer looks
//     at the key before it reads a parent): then a tile without a keyed pixel writes nothing, the others write only their keyed
//     pixels - the parents of background pixels stay stale;
//   * ws.area (STAT_AREA or STAT_SUMS), ws.sumy / ws.sumx (STAT_SUMS) and ws.flag hold a component's statistics at its ROOT's index.
//     flag bits, OR-ed over the component's pixels: AUX_BORDER bit0 = touches the image border, AUX_VALUE_EQ bit0 = holds a pixel
//     with value == aux_c, AUX_IMAGE bits 0-4 of aux_img[p], AUX_NONE 0.  A count_only pass writes none of them;
//   * ws.tile_any per 64 x 32 tile (index: tile_index): 0 no keyed pixel - later kernels skip the tile before they load anything of
//     it; 1 keyed pixels; 2 (allow_full only) every valid pixel is keyed, the tile is ONE component whose first pixel is its only
//     owner: only that pixel has a parent and stands in for every pixel of the tile, and the tile has no owner bits;
//   * ws.own_bits: 2048 bits per tile, bit (li & 31) of word li >> 5 = tile-local pixel li is an owner (never read where tile_any == 0);
//   * counters (G_*): CclPass::g null - the pass zeroes ws.g with a launch of its own and reduce_g_kernel folds the G_SHARDS replicas
//     into replica 0, which is what every consumer reads; CclPass::g set - the CALLER has zeroed the block and the consumers fold the
//     replicas themselves (g_fold_*).  A pass without counters (need == 0) touches none.
#pragma once
#include "common.h"
#include "device_util.h"

namespace ecseg {

typedef unsigned long long u64;

static constexpr uint32_t LUT_MULTI = 0x03020100u;   // key = value
static constexpr uint32_t LUT_NONZERO = 0xffffffffu; // key = (value != 0)
__host__ __device__ constexpr uint32_t lut_eq(int c) { return 1u << (8 * c); }                  // key = (value == c)
__host__ __device__ constexpr uint32_t lut_ne(int c) { return 0x01010101u & ~(0xffu << (8 * c)); }  // key = (value != c)
// key = (value != 0 && value != m)
__host__ __device__ constexpr uint32_t lut_nonzero_except(int m) { return 0x01010100u & ~(0xffu << (8 * m)); }

__device__ __forceinline__ int key_of(uint8_t v, uint32_t lut) {
    if (lut == LUT_NONZERO) return v != 0;
    return (lut >> ((v & 3) * 8)) & 0xff;
}

// per-image global counters.  The labelling kernels add into one of G_SHARDS replicas (each on its own 128-B line: thousands of
// workgroups of one image adding to ONE line serialise at ~60 ns per atomic, which used to cost ~1 ms per labelling);
// reduce_g_kernel folds the replicas into replica 0.
enum { G_NCOMP = 0 /*[4]*/, G_NPX = 4 /*[4]*/, G_LAST_ROOT = 8, G_NLIST1 = 9, G_NLIST2 = 10,
       G_CNT0 = 12 /* [8] generic root counters */, G_OTSU_INV = 20 };
enum { NEED_NCOMP = 1, NEED_NPX = 2, NEED_LAST = 4, NEED_LISTS = 8 };
static constexpr int G_IMG = G_STRIDE * G_SHARDS;     // ints per image

// aux modes of a pass: which per-pixel bits are OR-ed into the root's flag word
enum { AUX_NONE = 0, AUX_BORDER = 1, AUX_VALUE_EQ = 2, AUX_IMAGE = 3 };
enum { STAT_AREA = 1, STAT_SUMS = 2 };

// ---------------------------------------------------------------------------------------------------------------
// geometry helpers: a block = 4 waves; wave w owns the 64-pixel chunk `cx` of rows y0 + w*ROWS .. + ROWS-1
// ---------------------------------------------------------------------------------------------------------------
static constexpr int CCL_ROWS = 8;                      // rows per wave
static constexpr int CCL_BLOCK_ROWS = 4 * CCL_ROWS;     // rows per block

struct CclGeom {
    int H, W, n_img;
    int chunks_x, strips_y, blocks_per_img;
    int img_groups;   // n_img / 8: complete groups of 8 images, one image per XCD (see decode_block)
    int affine_blocks;   // 8 * img_groups * blocks_per_img: the workgroups of those groups; the rest deal the remaining images' tiles over all XCDs
};

inline CclGeom make_geom(int n_img, int H, int W) {
    CclGeom g;
    g.H = H; g.W = W; g.n_img = n_img;
    g.chunks_x = (W + 63) / 64;
    g.strips_y = (H + CCL_BLOCK_ROWS - 1) / CCL_BLOCK_ROWS;
    g.blocks_per_img = g.chunks_x * g.strips_y;
    g.img_groups = n_img / 8;
    g.affine_blocks = 8 * g.img_groups * g.blocks_per_img;
    return g;
}
inline unsigned geom_grid(const CclGeom& g) { return (unsigned)(g.n_img * g.blocks_per_img); }

// block id -> (image, strip, chunk).  Complete groups of 8 images: images with equal (img % 8) share an XCD (consecutive
// workgroups go to consecutive XCDs), so the parents, statistics and owner bits of an image stay in ONE L2 (64 images: 0.135 against
// 0.146 ms per speckled image with the tiles dealt round-robin).  The images beyond the last complete group - all of them when there are
// fewer than 8 - would leave XCDs idle that way (a single image ran its 726 tiles on 32 of the 256 CUs: 67 - 86 us per ccl_local
// launch; 9 images took 2x the time of 8): their tiles are dealt round-robin over all XCDs (round 4; every cross-tile access is an
// agent-scope atomic anyway: 9 images 0.223 -> 0.174 ms per speckled image, 12 images 0.179 -> 0.165).
__device__ __forceinline__ unsigned block_in_image(const CclGeom& g) {
    const unsigned b = blockIdx.x;
    return (b < (unsigned)g.affine_blocks ? (b >> 3) : b - (unsigned)g.affine_blocks) % (unsigned)g.blocks_per_img;
}
__device__ __forceinline__ bool decode_block(const CclGeom& g, int& img, int& y0, int& cx) {
    const unsigned b = blockIdx.x;
    if (b < (unsigned)g.affine_blocks) img = (int)(((b >> 3) / g.blocks_per_img) * 8 + (b & 7u));
    else img = 8 * g.img_groups + (int)((b - (unsigned)g.affine_blocks) / (unsigned)g.blocks_per_img);
    if (img >= g.n_img) return false;
    const unsigned blk = block_in_image(g);
    cx = (int)(blk % g.chunks_x);
    y0 = (int)(blk / g.chunks_x) * CCL_BLOCK_ROWS + (int)(threadIdx.x >> 6) * CCL_ROWS;
    return true;
}

// index of this block's tile in PostWorkspace::tile_any (valid after decode_block returned true)
__device__ __forceinline__ size_t tile_index(const CclGeom& g, int img) {
    return (size_t)img * g.blocks_per_img + block_in_image(g);
}

// the replica of image `img`'s counter block that this workgroup adds into
__device__ __forceinline__ int32_t* g_shard(int32_t* G_all, const CclGeom& g, int img) {
    return G_all + (size_t)img * G_IMG + (size_t)(block_in_image(g) % G_SHARDS) * G_STRIDE;
}

// consumers of a pass with its own counter block fold the replicas themselves (one thread, once per workgroup)
__device__ __forceinline__ int g_fold_sum(const int32_t* G_img, int idx) {
    int v = 0;
    for (int sh = 0; sh < G_SHARDS; ++sh) v += G_img[sh * G_STRIDE + idx];
    return v;
}
__device__ __forceinline__ int g_fold_max(const int32_t* G_img, int idx) {
    int v = 0;
    for (int sh = 0; sh < G_SHARDS; ++sh) v = max(v, G_img[sh * G_STRIDE + idx]);
    return v;
}

// The walk over a tile's owners, thread = 8 consecutive pixels of the tile (256 threads, one byte of the owner bits each):
//     uint32_t bits = thread_owner_bits(ta, own_bits, ti, tid);  while (bits) { const int p = pop_owner(bits, g, tid, yblk, cx); ... }
// A FULL tile (ta == 2: ccl_local wrote no owner bits for it) has one owner, its first pixel.  pop_owner takes the lowest bit and
// returns that owner's pixel index in the image (yblk: first row of the tile).
__device__ __forceinline__ uint32_t thread_owner_bits(int ta, const uint32_t* __restrict__ own_bits, size_t ti, int tid) {
    return ta == 2 ? (tid == 0 ? 1u : 0u) : (own_bits[ti * 64 + (tid >> 2)] >> ((tid & 3) * 8)) & 0xffu;
}
__device__ __forceinline__ int pop_owner(uint32_t& bits, const CclGeom& g, int tid, int yblk, int cx) {
    const int k = __ffs((int)bits) - 1;
    bits &= bits - 1;
    const int li = tid * 8 + k;
    return (yblk + (li >> 6)) * g.W + cx * 64 + (li & 63);
}

struct CclPass {
    const uint8_t* key_img;
    uint32_t lut;
    int conn;
    int stat;
    int aux_mode, aux_c;
    const uint8_t* aux_img;
    int need;      // NEED_* counters this pass has to produce
    bool count_only = false;   // only NEED_NCOMP | NEED_NPX are wanted: count roots instead of flattening
    bool sparse = false;       // every consumer checks the key before it reads a parent: background parents are not written
    bool allow_full = false;   // binary keys, 4-connectivity, no statistics / counters: tiles without an unkeyed pixel are one node (tile_any == 2)
    int32_t* list1 = nullptr;  // NEED_LISTS: per-image lists of class-1 roots / class-2 roots (first word of 16-byte slots)
    int32_t* list2 = nullptr;
    // ccl_resolve appends without looking at list_cap: NEED_LISTS is for conn == 8 only, where ceil(H/2) ceil(W/2) <= list_cap bounds
    // the roots of an image (a 4-connected checkerboard has twice as many); run_ccl_pass_debug's callers reject conn == 4 with lists.
    // The flag words of a count_only pass are not written (no slots): flag queries after one read stale words, rejected there too.
    size_t list_cap = 0;
    // counter block of this pass (null: ws.g, zeroed by a launch of its own and folded by reduce_g_kernel).  run_meta_inference
    // gives every labelling its own block, zeroes them all with ONE memset and lets the consumers fold the replicas themselves
    // (g_fold_*): two launches less per labelling
    int32_t* g = nullptr;
    // (round 5 tried to publish a count_only pass's result from the last workgroup of every image to finish - a ticket counter per
    // image: 726 workgroups x 64 images adding to ONE line per image made count_roots_kernel 25x slower (20 -> 546 us); the
    // per-image gather launch stays)
};
hipError_t run_ccl_pass(PostWorkspace& ws, const CclGeom& g, const CclPass& c, hipStream_t s);

// Up to 5 counts of roots by (key, flag bits) in ONE pass over the owner bits (count_flagged_owner_roots_kernel) after a pass on
// ws.g.  Query i: roots whose key == key[i] (0 = any) and whose flag word has all bits of need[i] -> G[G_CNT0 + slot[i]], folded
// into replica 0 by the reduce_g_kernel launch behind it.
struct FlagQueries { int n; int key[5]; uint32_t need[5]; int slot[5]; };
void launch_flagged_counts(PostWorkspace& ws, const CclGeom& g, const uint8_t* key_img, uint32_t lut, const FlagQueries& Q, hipStream_t s);

// The small kernels of ccl_kernels.hip that other files launch too, one launch each: zero_g_kernel over n ints of a counter range;
// gather_counts_kernel, G_NCOMP / G_NPX of `key` per image -> n_out / px_out (either may be null; fold != 0: the pass had a counter
// block of its own whose replicas nobody has folded yet)
void launch_zero_g(int32_t* G, int n, hipStream_t s);
void launch_gather_counts(const int32_t* G_all, int n_img, int key, int32_t* n_out, long long* px_out, long long full_px, int fold, hipStream_t s);

// ---- per-pixel kernels (one thread per pixel, grid-stride over the batch) --------------------------------------------------
inline unsigned px_grid(size_t total) {
    size_t b = (total + 255) / 256;
    if (b > 256 * 64) b = 256 * 64;
    return (unsigned)(b ? b : 1);
}
#define PX_LOOP(total) for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < (total); t += (size_t)gridDim.x * blockDim.x)
// The same over a batch with the image index in blockIdx.y (grid from img_grid): no 64-bit division per pixel to find the
// image a flat index belongs to.  Defines im (image), ib (its first flat index) and t (flat index) for the body.
#define IMG_PX_LOOP(n_img, px)                                                      \
    for (int im = blockIdx.y; im < (n_img); im += gridDim.y)                        \
        for (size_t ib = (size_t)im * (px), q_ = (size_t)blockIdx.x * blockDim.x + threadIdx.x, t = ib + q_; q_ < (px); \
             q_ += (size_t)gridDim.x * blockDim.x, t = ib + q_)
inline dim3 img_grid(size_t px, int n_img) {
    size_t bx = (px + 255) / 256;
    const size_t cap = (size_t)(256 * 64) / (size_t)(n_img > 0 ? (n_img < 16384 ? n_img : 16384) : 1);   // ~16 k blocks in all, several pixels per thread
    if (bx > cap) bx = cap;
    return dim3((unsigned)(bx ? bx : 1), (unsigned)(n_img < 65535 ? (n_img > 0 ? n_img : 1) : 65535));
}

}  // namespace ecseg
