// A-operand lane -> tile of the F(4x4) kernels: which of the workgroup's 32 Winograd tiles lane li of a wave half feeds to the MFMA.  Plain C++,
// included inside the kernel bodies and inside tools/lds_bank_model.cpp (lane_tile), which walks the LDS bank rule with this map.
// Expects: li (lane & 31); defines q8 (lane quad), tx (tile column), tg (region: W4_QUAD_REGION, wino4_lds_layout.h), ty (tile row = q8 >> 1).
    const int q8 = li >> 2, tx = li & 3;
    const int tg = W4_QUAD_REGION(q8);
    const int ty = (q8 == 0 || q8 == 1) ? 0 : (q8 == 2 || q8 == 3) ? 1 : (q8 == 4 || q8 == 5) ? 2 : 3;
