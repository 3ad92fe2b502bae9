// Constants, small helpers, hook defaults and schedule macros shared by the F(4x4) kernels (wino4_kernel.hip, wino4r_kernel.hip, wino4s_kernel.hip);
// included inside namespace ecseg.  What else the three share, each stated once:
//   wino4_lds_layout.h     W4Lds: every LDS size and address function; the region rule of the lane -> tile map (host-compilable)
//   wino4_lane_tile.inc    A-operand lane -> tile (also walked by tools/lds_bank_model.cpp)
//   wino4_region.inc       block order, the workgroup's two regions, halo LDS-DMA (dma_halo_piece)
//   wino4_filter_dma.inc   filter LDS-DMA (dma_filter_piece)
//   wino4_row_pass.inc      the row transform once per workgroup (row_pass; conv_wino4r / conv_wino4s) and its operation order
//   wino4_mfma_stage.inc   column transform + 12 fp32 MFMAs of one filter stage (mfma_stage; conv_wino4 / conv_wino4r)
//   wino4_fold.inc         the fold R = M[xi][:] A of one accumulator element (fp32 kernels)
//   wino4_out_begin.inc    start of the output stage (Rs, Cout, hl, the bias-quad prefetch bvp)
//   wino4_combine.inc / wino4_head.inc    the combine step of a channel-half pass, the fused head's tail

// Diagnostic hooks of the shared files.  The product build has ONE code path: every hook is empty.  A timing-only A/B build of one kernel
// (tools/w4r_variants.sh, tools/w4s_variants.sh) defines the ones it fills BEFORE this file is included; the shared files hold call sites only.
#ifndef W4_DIAG_SKIP_HALO_DMA
#define W4_DIAG_SKIP_HALO_DMA()                              // first statement of dma_halo_piece
#endif
#ifndef W4_DIAG_HALO_OFFSET
#define W4_DIAG_HALO_OFFSET(off, a)                          // after hoff[i] of LDS-DMA slot a is formed
#endif
#ifndef W4_DIAG_SKIP_FILTER_DMA
#define W4_DIAG_SKIP_FILTER_DMA()                            // first statement of dma_filter_piece
#endif
#ifndef W4_DIAG_FILTER_STAGE
#define W4_DIAG_FILTER_STAGE(stage) (stage)                  // the stage dma_filter_piece fetches
#endif

// Schedule macros of the K loops (a kernel's own phase macros - W4_TS / W4_SS, W4_S, W4_PH - are built from these)
#define W4_WAIT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define W4_BARRIER() asm volatile("s_barrier" ::: "memory")
#define W4_SB() __builtin_amdgcn_sched_barrier(0)
// the two barriers per group of conv_wino4r / conv_wino4s: Y (own share of the row pass is written), X (own t[] is loaded)
#define W4_Y() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); W4_BARRIER(); W4_SB(); } while (0)
#define W4_X() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); W4_BARRIER(); W4_SB(); } while (0)
#define W4_HALO(g) do { dma_halo_piece((g), std::integral_constant<int, 0>{}); dma_halo_piece((g), std::integral_constant<int, 1>{}); } while (0)

// Launch shared by launch_conv_wino4 / launch_conv_wino4r / launch_conv_wino4s (wino4_kernel.hip), after the caller's own eligibility checks:
// region count -> pairs -> grid of npairs * nblocks workgroups, span check, max(kloop_lds, exchange image) bytes of dynamic LDS.
struct DeviceOnce;
typedef void (*W4Kernel)(ConvParams, int, int, int);
hipError_t launch_wino4_grid(const ConvParams& p, hipStream_t s, W4Kernel kern, DeviceOnce& attr_set, size_t kloop_lds, int nblocks);

namespace {

// Every LDS size and lane -> address function of these kernels lives in wino4_lds_layout.h (W4Lds), which the including file
// includes at file scope; the names the launch functions use:
constexpr int W4_HS = W4Lds::HS;             // halo slots per raw buffer
constexpr int W4_BWS = W4Lds::BWS;           // filter slots per wave and stage (fp32 kernels)
constexpr int W4_RPLANE = W4Lds::RPLANE;     // floats per (xi, x) plane of the output exchange image

typedef __attribute__((address_space(3))) void* lptr_t;

// LDS-DMA (buffer_load ... lds for the halo, global_load_lds for the filter) is issued through inline asm on purpose: for the
// builtin the compiler orders every later ds_read behind the DMA with s_waitcnt vmcnt(0) (it cannot tell the LDS buffers
// apart), which serialises a stream that is interleaved with LDS reads.  The counted vmcnt waits in the kernel are the only
// ordering (the LDS destination is wave-uniform; M0 is restored).

// Interpolation points {0, +-a, +-b, inf} (common.h: W4_PA, W4_PB) and the constants of B^T and A^T they give:
//   B^T rows (monic Lagrange numerators): p = 0: [a2b2, 0, -(a2+b2), 0, 1, 0]      p = inf: [0, a2b2, 0, -(a2+b2), 0, 1]
//                                         p = +-a: [0, -+a b2, -b2, +-a, 1, 0]     p = +-b: [0, -+a2 b, -a2, +-b, 1, 0]
//   A^T = [1 1 1 1 1 0; 0 a -a b -b 0; 0 a2 a2 b2 b2 0; 0 a3 -a3 b3 -b3 1]
// All constants are exact in float32 for the dyadic points chosen.
constexpr float KA = (float)W4_PA, KB = (float)W4_PB, KA2 = KA * KA, KB2 = KB * KB, KA3 = KA2 * KA, KB3 = KB2 * KB;
constexpr float KP = KA2 * KB2, KS = -(KA2 + KB2);
static_assert((double)KA2 == W4_PA * W4_PA && (double)KB3 == W4_PB * W4_PB * W4_PB && (double)KP == W4_PA * W4_PA * W4_PB * W4_PB &&
              (double)KA3 == W4_PA * W4_PA * W4_PA && (double)(KA * KB2) == W4_PA * W4_PB * W4_PB && (double)(KA2 * KB) == W4_PA * W4_PA * W4_PB,
              "the Winograd points must keep every transform constant exact in float32");

}  // namespace
