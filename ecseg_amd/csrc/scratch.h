// Host-only: carves one device allocation (an arena) into typed slots.  Every slot starts on a multiple of 256 bytes from the
// base - the alignment hipMalloc gives - and a slot of zero elements is still a slot of its own.  The same code runs twice: with a
// null base it measures (`used` is the arena's size, the pointers are offsets), with the arena's base it places.  The layout
// functions of common.h (region_bufs, fishspot_bufs ...) are written against it and are the one statement of every buffer's size.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ecseg {
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(void* arena = nullptr) : base(reinterpret_cast<uintptr_t>(arena)) {}
    template <typename T>
    T* take(size_t n) { return reinterpret_cast<T*>(take_bytes(n * sizeof(T))); }
    virtual uintptr_t take_bytes(size_t bytes) {             // (virtual: the layout check derives a carver that records the slots)
        const size_t off = used;
        used += bytes ? (bytes + 255) / 256 * 256 : 256;
        return base + off;
    }
};
}  // namespace ecseg
