// Host-only: everything of an 8-bit LZW TIFF but its strips, shared by the host writer (tiff_write_u8, host_io.cpp) and the device
// encoder's drivers (ecseg_tiff_encode, drivers_files.hip; ecseg_fish_render_tiff, drivers_fish.hip).  A file is
//   head (8 bytes) | the strips back to back, a 0 after every strip of odd length | tail
// and the tail is: the strip offset and count tables (more than one strip), BitsPerSample (more than two samples), a pad byte to an
// even offset, the IFD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ecseg {

// strips of 8192 / (W * spp) rows, at least one row, at most the image (cv2.imwrite's rule)
inline int tiff_rows_per_strip(int H, int W, int spp) {
    const size_t line = (size_t)W * spp;
    int rps = (int)(8192 / line);
    if (rps < 1) rps = 1;
    if (rps > H) rps = H;
    return rps;
}
// what ecseg_lzw_encode never exceeds for a strip of n bytes: the capacity the host writer gives it, and the device encoder's slot
inline size_t tiff_strip_bound(size_t n) { return 2 * n + 64; }
// bytes of the tail (pad included or not: the larger) for a file of nstrips strips
inline size_t tiff_tail_bound(int nstrips, int spp) { return (nstrips > 1 ? 8 * (size_t)nstrips : 0) + (spp > 2 ? 2 * (size_t)spp : 0) + 1 + 2 + 12 * 12 + 4; }

// offs / cnts: file offset and byte count of every strip; data_end: the file offset behind the last strip (and its pad byte)
void tiff_frame(int H, int W, int spp, int rps, const uint32_t* offs, const uint32_t* cnts, int nstrips, size_t data_end,
                std::vector<uint8_t>* head, std::vector<uint8_t>* tail);

}  // namespace ecseg
