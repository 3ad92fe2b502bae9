// What the entry points of the drivers_*.hip files open and time themselves with, written once.  Macros where a step returns from
// the entry point (as HIP_TRY does), static functions for the rest (the library exports nothing of this file).  The macros spell their HIP calls with the caller's own names
// (`h`, `s`, the event numbers), so that the text HIP_TRY puts into a failure's message is what it was when each driver wrote them out.
#pragma once
#include "ctx.h"

// The opening of an entry point: no handle, no call; and any call but the next ecseg_meta_segment withdraws what was sent ahead.
#define DRIVER_OPEN(h) do { if (!h) return ECSEG_E_INVALID; drop_sent_ahead(h); } while (0)

// Before the first allocation, copy or launch.  Validation that needs no device stands in front of it.
#define USE_DEVICE(h) HIP_TRY(h, hipSetDevice(h->device))

// A timed region on stream s: ev[a], the launches (statements; they may return, as HIP_TRY does), ev[b]: the kernels alone, inputs
// resident.  Their device time is read once the stream has been waited for: WAIT_SET / WAIT_ADD wait and then put it into stage_ms
// (ECSEG_T_COUNT of ecseg_get_timings); timed_set / timed_add do the second half where the wait is elsewhere or the stage another.
// `set` where the call has one region; `add` in a chunk loop and for the FISH drivers' second region (ev[2], ev[3]).
#define TIMED(h, s, a, b, ...) do { HIP_TRY(h, hipEventRecord(h->ev[a], s)); __VA_ARGS__; HIP_TRY(h, hipEventRecord(h->ev[b], s)); } while (0)
#define WAIT_SET(h, s, a, b) do { HIP_TRY(h, hipStreamSynchronize(s)); timed_set(h, a, b); } while (0)
#define WAIT_ADD(h, s, a, b) do { HIP_TRY(h, hipStreamSynchronize(s)); timed_add(h, a, b); } while (0)

namespace ecseg {

static inline void timed_set(ecseg_ctx* h, int a, int b, int stage = ECSEG_T_COUNT) { h->stage_ms[stage] = stage_elapsed(h->ev[a], h->ev[b]); }
static inline void timed_add(ecseg_ctx* h, int a, int b, int stage = ECSEG_T_COUNT) { h->stage_ms[stage] += stage_elapsed(h->ev[a], h->ev[b]); }

// ecseg_get_timings shows zeros from here on, also after a later step of the call has failed: each driver keeps its own moment.
static inline void clear_timings(ecseg_ctx* h) { for (float& v : h->stage_ms) v = 0.f; }

// Pixel indices fit an int: the kernels count H * W in 32 bits.  The refusal's message is the caller's.
static inline bool px_below_2_31(int H, int W) { return (long long)H * W < (1ll << 31); }

}  // namespace ecseg
