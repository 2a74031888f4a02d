// stream_pool.h -- the streams of a chain handle, kept per process: a handle takes a set when it is created and gives it
// back when it is destroyed (stream_pool.cpp: why, and what was measured).
#pragma once

#include <hip/hip_runtime.h>

#ifndef XRIT_WALK_STREAMS
#define XRIT_WALK_STREAMS 2
#endif

namespace xrit {

struct StreamSet {
    int device = -1;
    hipStream_t s = nullptr, s2 = nullptr, s3[XRIT_WALK_STREAMS] = {}, sc = nullptr;
};

// a stream with a hardware queue of its own (XRIT_SHARED_QUEUES=1: plain hipStreamCreate)
hipError_t create_own_queue_stream(hipStream_t *s);
// a set of the pool on `device`, or a new one; false: a stream could not be created
bool stream_set_acquire(int device, StreamSet *out);
// waits for the set's streams and keeps them for the next handle on that device (nothing is destroyed)
void stream_set_release(const StreamSet &st);

}  // namespace xrit
