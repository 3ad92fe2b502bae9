// Per-cell device primitives shared by the interSeg regions, the FISH distances, the FISH spot statistics and the watershed
// clean-up and rescale (interseg_kernels.hip, fishdist_kernels.hip, fishspot_kernels.hip, watershed_kernels.hip, rescale_kernels.hip; gfx950 only).  Everything
// built from them is an integer sum, OR, minimum, maximum or root count, so no result depends on the order of the atomics.
#pragma once
#include "device_util.h"

namespace ecseg {

typedef unsigned long long u64;

static constexpr int CELL_SLOTS = 64;            // entries of the LDS key table
static constexpr int CELL_ROWS_PER_WAVE = 8;     // statistics tile: 64 columns x 32 rows (4 waves x 8 rows)
static constexpr int CELL_CHUNK = 1024;          // elements per scan chunk (256 threads x 4)

// ---- the lanes of one key -------------------------------------------------------------------------------------------------
// f(key, mine, mask, leader) once per distinct key >= 0 among the 64 lanes, starting from the lowest active lane: `mine` = this
// lane holds `key`, `mask` = the ballot of those lanes, `leader` = the lowest of them.  Call it wave-uniformly.
template <class F>
__device__ __forceinline__ void wave_key_groups(int key, F&& f) {
    u64 active = __ballot(key >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int group = __shfl(key, leader);
        const bool mine = key == group;
        const u64 m = __ballot(mine);
        f(group, mine, m, leader);
        active &= ~m;
    }
}

// The slot of `key` in a CELL_SLOTS-entry LDS table preset to -1 (linear probing), or -1 when the table holds CELL_SLOTS other
// keys: the caller then adds straight to the cell's global accumulators.  Payload arrays and flush are the kernel's own.
__device__ __forceinline__ int lds_key_claim(int* s_key, int key) {
    int slot = key & (CELL_SLOTS - 1);
    for (int probe = 0; probe < CELL_SLOTS; ++probe) {
        const int old = atomicCAS(&s_key[slot], -1, key);
        if (old == -1 || old == key) return slot;
        slot = (slot + 1) & (CELL_SLOTS - 1);
    }
    return -1;
}

// The statistics tile of workgroup blockIdx.x (256 threads, 1-D grid of stat_tiles(H, W)): a wave walks rows ybeg .. ybeg + 7 of
// the columns xb .. xb + 63, lane = column.  x < W + 63 <= 2^31 + 62: compare it as unsigned.
struct StatTile { unsigned xb, x; int ybeg; };
__device__ __forceinline__ StatTile stat_tile(int W) {
    const unsigned tiles_x = ((unsigned)W + 63u) / 64u;
    const unsigned xb = (blockIdx.x % tiles_x) * 64u;
    return StatTile{xb, xb + (threadIdx.x & 63u),
                    (int)(blockIdx.x / tiles_x) * (4 * CELL_ROWS_PER_WAVE) + (int)(threadIdx.x >> 6) * CELL_ROWS_PER_WAVE};
}
// ... and of tile `tile` of an image that shares its grid with others (fishdist_batch.h: the workgroup looks its image up first)
__device__ __forceinline__ StatTile stat_tile_at(unsigned tile, int W) {
    const unsigned tiles_x = ((unsigned)W + 63u) / 64u;
    const unsigned xb = (tile % tiles_x) * 64u;
    return StatTile{xb, xb + (threadIdx.x & 63u), (int)(tile / tiles_x) * (4 * CELL_ROWS_PER_WAVE) + (int)(threadIdx.x >> 6) * CELL_ROWS_PER_WAVE};
}
inline unsigned stat_tiles(int H, int W) {
    return (((unsigned)W + 63u) / 64u) * (((unsigned)H + 4 * CELL_ROWS_PER_WAVE - 1) / (4 * CELL_ROWS_PER_WAVE));
}

// ---- exclusive scan -------------------------------------------------------------------------------------------------------
// The scanned sequence is load(0), load(1), ..., load(n - 1) of a small functor:
struct LoadStrided {                             // v[i * stride]
    const int32_t* v; int stride;
    __device__ int operator()(size_t i) const { return v[i * stride]; }
};
struct LoadRootFlag {                            // 1 where pixel i is the first pixel of its component (label = 1 + raster index)
    const int32_t* L;
    __device__ int operator()(size_t i) const { return L[i] == (int)i + 1; }
};

// blk[chunk] = sum of the chunk's elements
template <class Load>
__global__ __launch_bounds__(256) void scan_chunk_sum_kernel(Load load, int n, int32_t* __restrict__ blk) {
    __shared__ int wsum[4];
    const int t = threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * CELL_CHUNK + (size_t)t * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += i0 + k < (size_t)n ? load(i0 + k) : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive prefix over the chunk sums (one workgroup, 256 chunks per pass with a carry); *total = their sum
static __global__ __launch_bounds__(256) void scan_blocks_kernel(int32_t* __restrict__ blk, int nb, int32_t* __restrict__ total) {
    __shared__ int s[256];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int i = b0 + t;
        const int v = i < nb ? blk[i] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int a = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (i < nb) blk[i] = carry + s[t] - v;
        __syncthreads();
        if (t == 255) carry += s[255];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

// out[i] = sum of load(j) over j < i (out may be the array `load` reads at stride 1: a thread reads its four elements first)
template <class Load>
__global__ __launch_bounds__(256) void scan_chunk_excl_kernel(Load load, int n, const int32_t* __restrict__ blk, int32_t* out) {
    __shared__ int wsum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t i0 = (size_t)blockIdx.x * CELL_CHUNK + (size_t)t * 4;
    int a[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = i0 + k < (size_t)n ? load(i0 + k) : 0; s += a[k]; }
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int run = blk[blockIdx.x] + incl - s;
#pragma unroll
    for (int w = 0; w < 4; ++w) run += w < wv ? wsum[w] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < (size_t)n) out[i0 + k] = run;
        run += a[k];
    }
}

// out[i] = load(0) + ... + load(i - 1) for i < n, *total = the sum of all; blk: ceil(n / CELL_CHUNK) int32 of scratch
template <class Load>
inline void exclusive_scan(Load load, int n, int32_t* blk, int32_t* out, int32_t* total, hipStream_t s) {
    const int nb = (int)(((unsigned)n + CELL_CHUNK - 1) / CELL_CHUNK);
    hipLaunchKernelGGL(scan_chunk_sum_kernel<Load>, dim3(nb), dim3(256), 0, s, load, n, blk);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, blk, nb, total);
    hipLaunchKernelGGL(scan_chunk_excl_kernel<Load>, dim3(nb), dim3(256), 0, s, load, n, blk, out);
}

// ---- connected components over uf_unite (device_util.h) -------------------------------------------------------------------
// Unite pixel p = (y, x), itself keyed (parent >= 0), with its W and N and, conn8, NW and NE neighbour q where same(q) holds and
// q is keyed.  Parents only ever move to smaller pixel indices, so "was preset to a pixel" stays readable as >= 0 while other
// threads unite.
template <class Same>
__device__ __forceinline__ void uf_unite_back(int32_t* par, int p, int y, int x, int W, int conn8, Same&& same) {
    auto link = [&](int q) { if (same(q) && uf_load(par, q) >= 0) uf_unite(par, p, q); };
    if (x > 0) link(p - 1);
    if (y > 0) {
        link(p - W);
        if (conn8) {
            if (x > 0) link(p - W - 1);
            if (x + 1 < W) link(p - W + 1);
        }
    }
}

// Pixel pu of one plane of par / sz (px entries each): parent = root for a keyed pixel, sz[root] = pixels of the component.
// cnt (may be null): [0] += components, [1] += keyed pixels.  Call it with whole waves (the counters are summed by ballot).
__device__ __forceinline__ void uf_size_pixel(int px, int32_t* par, int32_t* __restrict__ sz, int32_t* __restrict__ cnt, unsigned pu) {
    const int p = (int)pu;
    bool keyed = false, is_root = false;
    if (pu < (unsigned)px && uf_load(par, p) >= 0) {
        keyed = true;
        const int root = uf_find(par, p);
        __hip_atomic_store(par + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a shortcut inside the same tree
        atomicAdd(sz + root, 1);
        is_root = root == p;
    }
    if (cnt) {                                               // one atomic per wave and counter
        const int nk = __popcll(__ballot(keyed)), nr = __popcll(__ballot(is_root));
        if ((threadIdx.x & 63) == 0) {
            if (nr) atomicAdd(cnt + 0, nr);
            if (nk) atomicAdd(cnt + 1, nk);
        }
    }
}

// Plane blockIdx.y of par / sz (px entries each); cnt: one plane only.
static __global__ __launch_bounds__(256) void uf_size_kernel(int px, int32_t* par_all, int32_t* __restrict__ sz_all,
                                                             int32_t* __restrict__ cnt) {
    const size_t o = (size_t)blockIdx.y * (size_t)px;
    uf_size_pixel(px, par_all + o, sz_all + o, cnt, blockIdx.x * 256u + threadIdx.x);   // px < 2^31: no wrap
}

// ---- the dense cell index -------------------------------------------------------------------------------------------------
// Pixel p of a label map of px pixels: flag[label - 1] = 1 for a label that occurs; *bad = 1 when a label exceeds px (the caller
// refuses the map).  An exclusive scan over flag then gives every label its dense ascending cell index.
__device__ __forceinline__ void cell_mark_pixel(const int32_t* __restrict__ L, int px, int32_t* __restrict__ flag, int32_t* __restrict__ bad,
                                                unsigned p) {
    if (p >= (unsigned)px) return;
    const int l = L[p];
    if (l <= 0) return;
    if (l > px) { *bad = 1; return; }
    flag[l - 1] = 1;
}

}  // namespace ecseg
