// Constants and small helpers shared by the F(4x4) kernels (wino4_kernel.hip, wino4r_kernel.hip, wino4s_kernel.hip); included inside namespace ecseg.
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
