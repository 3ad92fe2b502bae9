// The fold R = M[xi][:] A of one accumulator element of the fp32 kernels, included inside the element loop of a fold: the six points of the
// wave's transform row -> the four values of the exchange image.  (conv_wino4s_kernel folds HALF rows: other arithmetic, its own.)
// Expects: acc[6], e, Rs, fold_at (the element's float index in the exchange image: W4Lds::r_fold / r_fold_tile); defines o, r0, r1, r2, r3.
            const float m0 = acc[0][e], m1 = acc[1][e], m2 = acc[2][e], m3 = acc[3][e], m4 = acc[4][e], m5 = acc[5][e];
            const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
            float* o = Rs + fold_at;
            const float r0 = m0 + s12 + s34, r1 = __builtin_fmaf(KA, d12, KB * d34), r2 = __builtin_fmaf(KA2, s12, KB2 * s34),
                        r3 = __builtin_fmaf(KA3, d12, __builtin_fmaf(KB3, d34, m5));
