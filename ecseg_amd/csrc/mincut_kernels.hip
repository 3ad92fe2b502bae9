// ecseg_min_cut: a batch of independent unit-capacity grid max-flows, one workgroup per task (src/max_flow_binary_mask.py:59-116).
//
// The network is the one of get_graph (:59-72) as include/ecseg_hip.h restates it.  The answer - the set reachable from the source
// in the residual network of a maximum flow - is the same for every maximum flow, so the augmentation order is free.  Each PHASE
// runs one complete breadth-first search from the source over the residual arcs (a queue of pixel indices, one level per
// barrier interval, every pixel claimed once with an atomic OR on its mark byte), then augments along SEVERAL paths at once:
// every pixel that still has room into the sink follows its parent marks back to the child of the source it hangs under, one
// candidate per such child is kept, and the kept paths - they lie in different subtrees of the search tree, so they share no
// pixel and hence no arc - are pushed concurrently, one lane each.  A phase that finds no candidate has left the reachable
// set in the marks: that is `side`.  At most 2 d (d + 1) + 1 phases (the source has that many arcs).
//
// State per pixel: a flow byte (bit 7 body pixel; bits 0-1 net flow to the right neighbour + 1; bits 2-3 net flow to the lower
// neighbour + 1; bit 4 flow on the arc from the source; bits 5-6 flow into the sink, 0..2) and a mark byte (bit 7 visited,
// bits 0-2 where the search came from: 1 left, 2 right, 3 above, 4 below, 5 the source), plus a queue slot.  Windows of up to
// ECSEG_MIN_CUT_LDS_PIXELS pixels keep all three in LDS (4 bytes per pixel, 16-bit queue), larger ones in a global scratch
// region of the call (6 bytes per pixel).  Net flows of two body pixels stay in {-1, 0, 1}: two anti-parallel unit arcs.
#include "common.h"

namespace ecseg {
namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_LDS = ECSEG_MIN_CUT_LDS_PIXELS;
constexpr int MC_SIDE = 2 * ECSEG_MIN_CUT_MAX_DIST + 1;
constexpr unsigned F_BODY = 0x80u, F_SRC = 0x10u, F_SINK1 = 0x20u, F_ZERO = 0x05u;   // F_ZERO: both net flows 0
constexpr unsigned B_SEEN = 0x80u, B_FROM_SRC = 5u;

struct McShared { int head, tail, aug, flow; };

__device__ __forceinline__ int parent_of(int p, unsigned from, int w) {
    return from == 1u ? p - 1 : from == 2u ? p + 1 : from == 3u ? p - w : p + w;
}

// Claims q for the search tree; `from` says on which side of q the pixel that reached it lies.
template <typename QT>
__device__ __forceinline__ void mc_visit(int q, unsigned from, const uint8_t* F, uint32_t* Bw, QT* Q, McShared* sh) {
    if (!(F[q] & F_BODY)) return;
    uint32_t* word = Bw + (q >> 2);
    const int shift = (q & 3) * 8;
    if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> shift) & B_SEEN) return;
    const uint32_t old = __hip_atomic_fetch_or(word, B_SEEN << shift, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if ((old >> shift) & B_SEEN) return;
    __hip_atomic_fetch_or(word, from << shift, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const int slot = __hip_atomic_fetch_add(&sh->tail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    Q[slot] = (QT)q;
}

// One task on the calling workgroup.  F, Bw (as bytes) and Q hold h * w entries each (Bw rounded up to whole words).
template <typename QT>
__device__ __forceinline__ void mc_task(const uint8_t* M, int h, int w, int sy, int sx, int ty, int tx, int d, uint8_t* F, uint32_t* Bw,
                                        QT* Q, int* claim, McShared* sh, uint8_t* side, int32_t* flow_out) {
    const int n = h * w, tid = threadIdx.x, S = sy * w + sx, T = ty * w + tx;
    const uint8_t* B = reinterpret_cast<const uint8_t*>(Bw);
    uint8_t* Bbyte = reinterpret_cast<uint8_t*>(Bw);
    const int ball = 2 * d + 1, ball2 = ball * ball;
    for (int i = tid; i < n; i += MC_THREADS) F[i] = (M[i] && i != S && i != T) ? (uint8_t)(F_BODY | F_ZERO) : (uint8_t)0;
    if (tid == 0) sh->flow = 0;
    const int max_phases = 2 * d * (d + 1) + 1;
    for (int phase = 0; phase < max_phases; ++phase) {
        for (int i = tid; i < (n + 3) / 4; i += MC_THREADS) Bw[i] = 0u;
        for (int i = tid; i < ball2; i += MC_THREADS) claim[i] = -1;
        if (tid == 0) { sh->head = 0; sh->tail = 0; sh->aug = 0; }
        __syncthreads();
        // the children of the source: body pixels of its ball whose arc is still empty
        for (int k = tid; k < ball2; k += MC_THREADS) {
            const int dy = k / ball - d, dx = k % ball - d, y = sy + dy, x = sx + dx;
            if (abs(dy) + abs(dx) > d || y < 0 || y >= h || x < 0 || x >= w) continue;
            const int p = y * w + x;
            const unsigned f = F[p];
            if (!(f & F_BODY) || (f & F_SRC)) continue;
            Bbyte[p] = (uint8_t)(B_SEEN | B_FROM_SRC);
            Q[__hip_atomic_fetch_add(&sh->tail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = (QT)p;
        }
        for (;;) {                                            // one level of the search per round
            __syncthreads();
            const int lo = sh->head, hi = sh->tail;
            __syncthreads();
            if (lo == hi) break;
            if (tid == 0) sh->head = hi;
            for (int i = lo + tid; i < hi; i += MC_THREADS) {
                const int p = (int)Q[i], y = p / w, x = p - y * w;
                const unsigned f = F[p];
                if (x + 1 < w && (f & 3u) < 2u) mc_visit(p + 1, 1u, F, Bw, Q, sh);
                if (x > 0 && (F[p - 1] & 3u) > 0u) mc_visit(p - 1, 2u, F, Bw, Q, sh);
                if (y + 1 < h && ((f >> 2) & 3u) < 2u) mc_visit(p + w, 3u, F, Bw, Q, sh);
                if (y > 0 && ((F[p - w] >> 2) & 3u) > 0u) mc_visit(p - w, 4u, F, Bw, Q, sh);
            }
        }
        // pixels with room into the sink: those of its ball outside the source's ball (one arc) and its 4-neighbours (one more)
        for (int pass = 0; pass < 2; ++pass) {
            for (int k = tid; k < ball2; k += MC_THREADS) {
                const int dy = k / ball - d, dx = k % ball - d, y = ty + dy, x = tx + dx;
                const int r = abs(dy) + abs(dx);
                if (r > d || y < 0 || y >= h || x < 0 || x >= w) continue;
                const int p = y * w + x;
                const unsigned f = F[p];
                if (!(f & F_BODY) || !(B[p] & B_SEEN)) continue;
                const unsigned cap = (abs(y - sy) + abs(x - sx) > d ? 1u : 0u) + (r == 1 ? 1u : 0u);
                if (((f >> 5) & 3u) >= cap) continue;
                int cur = p;
                unsigned from;
                while ((from = B[cur] & 7u) != B_FROM_SRC) cur = parent_of(cur, from, w);
                const int ry = cur / w, rx = cur - ry * w;
                int* mine = claim + (ry - sy + d) * ball + (rx - sx + d);
                if (pass == 0) {
                    __hip_atomic_store(mine, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
                if (*mine != p) continue;
                F[p] = (uint8_t)(f + F_SINK1);
                cur = p;
                while ((from = B[cur] & 7u) != B_FROM_SRC) {    // one more unit from the parent into cur
                    const int q = parent_of(cur, from, w);
                    if (from == 1u) F[q] += 1;
                    else if (from == 2u) F[cur] -= 1;
                    else if (from == 3u) F[q] += 4;
                    else F[cur] -= 4;
                    cur = q;
                }
                F[cur] |= (uint8_t)F_SRC;
                __hip_atomic_fetch_add(&sh->aug, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
        }
        const int pushed = sh->aug;
        __syncthreads();
        if (tid == 0) sh->flow += pushed;
        if (pushed == 0) break;
    }
    __syncthreads();
    for (int i = tid; i < n; i += MC_THREADS) side[i] = (i == S || (B[i] & B_SEEN)) ? (uint8_t)1 : (uint8_t)0;
    if (tid == 0) *flow_out = sh->flow;
}

// desc: per task (mask offset, h, w, sy, sx, ty, tx, 0); soff: byte offset of the task's region in `scratch`, < 0 = state in LDS.
// Both kernels are launched over all tasks; a workgroup whose task belongs to the other kernel returns at once.
__global__ __launch_bounds__(MC_THREADS) void mincut_lds_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ desc,
                                                                const long long* __restrict__ soff, int d, uint8_t* __restrict__ side,
                                                                int32_t* __restrict__ flow) {
    __shared__ uint32_t s_f[MC_LDS / 4], s_b[MC_LDS / 4];
    __shared__ uint16_t s_q[MC_LDS];
    __shared__ int s_claim[MC_SIDE * MC_SIDE];
    __shared__ McShared s_sh;
    if (soff[blockIdx.x] >= 0) return;
    const int32_t* t = desc + 8 * (size_t)blockIdx.x;
    const size_t off = (size_t)t[0];
    mc_task<uint16_t>(masks + off, t[1], t[2], t[3], t[4], t[5], t[6], d, reinterpret_cast<uint8_t*>(s_f), s_b, s_q, s_claim, &s_sh, side + off,
                      flow + blockIdx.x);
}

__global__ __launch_bounds__(MC_THREADS) void mincut_global_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ desc,
                                                                   const long long* __restrict__ soff, int d, uint8_t* scratch,
                                                                   uint8_t* __restrict__ side, int32_t* __restrict__ flow) {
    __shared__ int s_claim[MC_SIDE * MC_SIDE];
    __shared__ McShared s_sh;
    const long long so = soff[blockIdx.x];
    if (so < 0) return;
    const int32_t* t = desc + 8 * (size_t)blockIdx.x;
    const size_t off = (size_t)t[0], n4 = ((size_t)t[1] * t[2] + 3) / 4 * 4;
    uint8_t* base = scratch + so;
    mc_task<uint32_t>(masks + off, t[1], t[2], t[3], t[4], t[5], t[6], d, base, reinterpret_cast<uint32_t*>(base + n4),
                      reinterpret_cast<uint32_t*>(base + 2 * n4), s_claim, &s_sh, side + off, flow + blockIdx.x);
}

}  // namespace

size_t mincut_scratch_bytes(int h, int w) {
    const size_t n4 = ((size_t)h * w + 3) / 4 * 4;
    return (2 * n4 + 4 * (size_t)h * w + 15) / 16 * 16;
}

hipError_t run_mincut(const uint8_t* masks, const int32_t* desc, const long long* soff, int n_tasks, int n_global, int d, uint8_t* scratch,
                      uint8_t* side, int32_t* flow, hipStream_t s) {
    if (n_tasks <= 0) return hipSuccess;
    if (n_global < n_tasks)
        hipLaunchKernelGGL(mincut_lds_kernel, dim3((unsigned)n_tasks), dim3(MC_THREADS), 0, s, masks, desc, soff, d, side, flow);
    if (n_global > 0)
        hipLaunchKernelGGL(mincut_global_kernel, dim3((unsigned)n_tasks), dim3(MC_THREADS), 0, s, masks, desc, soff, d, scratch, side, flow);
    return hipGetLastError();
}

}  // namespace ecseg
