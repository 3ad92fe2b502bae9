// Host and device: what ecseg_classify_nucleus_crops (drivers_interseg.hip) and iseg_classifier_inputs_kernel (interseg_kernels.hip)
// share with the host program that checks them (tools/asan/iseg_classify_check.cpp) - the per-element arithmetic of the ecSeg-c
// input, the rules that choose the crops each classifier sees, and the chunks the crops travel in.
//
// ecSeg-c input (src/utils.py:166-173, interseg.preprocess_ecseg_c): per channel c of a crop, norm = (float)max_c of that crop and
//   value = rint((x / norm) * 255.0f) / 255.0f
// in float32, each operation rounded on its own (IEEE division, half to even; the files that include this are compiled without
// contraction and nothing here is a reciprocal).  norm == 0 gives 0 / 0 = NaN, as numpy and the reference give.
// ecSeg-i input: (float)x of channel 0, what u8_to_f32_kernel makes of crops[..., 0].
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISEG_HD __host__ __device__ __forceinline__
#else
#define ISEG_HD inline
#endif

namespace ecseg {

constexpr int ISEG_CHUNK = 256;                 // crops per launch of the crop kernel: 48 MiB of crops
constexpr int ISEG_CENT_GATE = 10;              // ecSeg-c sees a crop whose probe channel maximum is ABOVE this (src/interseg.py:160)

ISEG_HD float iseg_c_norm(int32_t channel_max) { return (float)channel_max; }
ISEG_HD float iseg_c_quant(uint32_t x, float norm) {
    const float q = (float)x / norm;
    const float s = q * 255.0f;
    return rintf(s) / 255.0f;
}
// the per-element function: sample x of a channel whose maximum over the crop is channel_max
ISEG_HD float iseg_c_value(uint32_t x, int32_t channel_max) { return iseg_c_quant(x, iseg_c_norm(channel_max)); }

// ---- host side: selection and chunks -------------------------------------------------------------------------------------------
// Crops travel in chunks of ISEG_CHUNK; a chunk's selected crops run through a model in sub-chunks of at most that model's windows
// per group.
inline int iseg_chunk_count(int n) { return n <= 0 ? 0 : (n + ISEG_CHUNK - 1) / ISEG_CHUNK; }
inline int iseg_chunk_len(int n, int chunk) { const int left = n - chunk * ISEG_CHUNK; return left < ISEG_CHUNK ? left : ISEG_CHUNK; }
inline int iseg_sub_count(int n_sel, int per_group) { return n_sel <= 0 ? 0 : (n_sel + per_group - 1) / per_group; }
inline int iseg_sub_len(int n_sel, int per_group, int sub) { const int left = n_sel - sub * per_group; return left < per_group ? left : per_group; }

// The rules of interseg.classify_crops for the k crops of one chunk: ecSeg-i runs for every crop but a from_patches crop whose three
// maxima are all 0 (an empty tile of an oversized nucleus); ecSeg-c for a crop that ecSeg-i runs for, when the image is
// `centromeric` (a centromeric model and a passed quality score) and the crop's probe channel (1) is brighter than the gate.
// sel_i / sel_c: the chosen crops' indices within the chunk, ascending (room for k each); ran_i / ran_c: one byte per crop.
inline void iseg_select(const int32_t* max3, const uint8_t* from_patches, int k, int centromeric, int32_t* sel_i, int* n_i, int32_t* sel_c,
                        int* n_c, uint8_t* ran_i, uint8_t* ran_c) {
    int ni = 0, nc = 0;
    for (int j = 0; j < k; ++j) {
        const int32_t* m = max3 + (size_t)j * 3;
        const bool empty = from_patches[j] && m[0] == 0 && m[1] == 0 && m[2] == 0;
        const bool c = !empty && centromeric && m[1] > ISEG_CENT_GATE;
        ran_i[j] = empty ? 0 : 1;
        ran_c[j] = c ? 1 : 0;
        if (!empty) sel_i[ni++] = j;
        if (c) sel_c[nc++] = j;
    }
    *n_i = ni; *n_c = nc;
}

}  // namespace ecseg
