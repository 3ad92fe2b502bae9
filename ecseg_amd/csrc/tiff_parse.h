// Host-only: the TIFF parser of the native reader (parse_tiff, host_io.cpp) for the drivers, as tiff_frame.h serves the encoder: the
// device reader (ecseg_tiff_decode, drivers.hip) reads the same tags by the same rules as ecseg_tiff_info / ecseg_tiff_read, and
// the one rule that says which files it takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ecseg {

struct TiffInfo {
    uint32_t W = 0, H = 0, bits = 8, spp = 1, comp = 1, planar = 1, pred = 1, fmt = 1, rps = 0;
    std::vector<uint32_t> off, cnt;
    bool le = true;
};

// ECSEG_OK, ECSEG_E_UNSUPPORTED (a valid layout this reader leaves to the Python one) or ECSEG_E_INVALID (corrupt)
int parse_tiff(const uint8_t* buf, size_t n, TiffInfo* t);

// The routing rule of the device reader, the only place that decides whether a file goes to the device (ecseg_tiff_decode_routes
// asks it for image_io.imread; ecseg_tiff_decode itself decodes whatever it is given).  A strip is one serial LZW stream on one
// wave, about 0.8 us per decoded byte on noisy data against 2.6 ns on a host core: the device wins by the number of strips that
// decode at once.  The threshold is the measurement of DESIGN.md 5.9 (tools/time_tiff_decode.py, a 1040 x 1392 RGB scene): the
// device call is faster than ecseg_tiff_read at 1040 strips (3.8 against 11.2 ms) and slower at 208 (14.0 against 11.1 ms), at 70, at
// 17 and at 1; 1040 is the smallest count measured at which it wins.  Uncompressed strips lose on the device (6.9 against 1.3 ms:
// the copies to and from the device cost more than the host's one memcpy) and Deflate has no device decoder: both stay on the host.
constexpr size_t TIFF_DEVICE_MIN_STRIPS = 1040;
inline bool tiff_goes_to_device(const TiffInfo& t) {
    if (t.comp != 5 || t.rps == 0) return false;
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps;
    return nstrips >= TIFF_DEVICE_MIN_STRIPS && t.off.size() >= nstrips;
}

}  // namespace ecseg
