// Timing-only ablations of conv_wino4s_kernel, compiled in only by tools/w4s_variants.sh (-DECSEG_W4S_ABL=<bits>; results are garbage):
//   1 no filter DMA   2 no halo DMA   4 no MFMAs   8 no split arithmetic   16 every filter stage read from the wave's first one (hot in
//   cache)   32 every halo piece one contiguous KB.  Numbers: EXPERIMENTS.md (round 6), gpurun_out/r06_w4s_*ablate*.log.
#define W4_DIAG_SKIP_HALO_DMA() do { if (ECSEG_W4S_ABL & 2) return; } while (0)
#define W4_DIAG_HALO_OFFSET(off, a) do { if (ECSEG_W4S_ABL & 32) off = (unsigned)(a) * 16u; } while (0)
#define W4_DIAG_SKIP_FILTER_DMA() do { if (ECSEG_W4S_ABL & 1) return; } while (0)
#define W4_DIAG_FILTER_STAGE(stage) ((ECSEG_W4S_ABL & 16) ? 0 : (stage))
#define W4S_DIAG_NO_SPLIT ((ECSEG_W4S_ABL & 8) != 0)
#if ECSEG_W4S_ABL & 4
#define W4S_MFMA(CB, A, B) asm volatile("" :: "v"(A), "v"(B))
#else
#define W4S_MFMA(CB, A, B) acc[P][CB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[P][CB], 0, 0, 0)
#endif
