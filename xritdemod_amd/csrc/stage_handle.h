// stage_handle.h -- what the stateful handles (framer, lock, decoder, demux, packets, files, images; the first three through
// frame_cores.h) share on the host: the device, the
// host-buffer path's own stream, the stream of the most recent call, and the "summary, written prefixes, XRIT_E_CAPACITY"
// tail of a host-buffer call with capacities.  Host only.
#pragma once

#include <initializer_list>
#include <new>
#include <string>

#include "common.h"

namespace xrit {

struct StageHandle {
    int device = 0;
    hipStream_t stream = nullptr;           // the host-buffer path's
    hipStream_t last_stream = nullptr;      // the stream of the most recent call: the state's last writer

    int open(int dev)
    {
        XR_TRY(select_device(dev));
        device = dev;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed");
            stream = nullptr;
            return XRIT_E_HIP;
        }
        last_stream = stream;
        return XRIT_OK;
    }
    // every wait comes before the own stream is destroyed (last_stream may be that stream); the buffers go last
    void close(std::initializer_list<DevBuf *> bufs = {})
    {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            if (last_stream != stream) (void)hipStreamSynchronize(last_stream);
            (void)hipStreamDestroy(stream);
            stream = last_stream = nullptr;
        }
        for (DevBuf *b : bufs) b->release();
    }
    // in front of anything that reads or rewrites the state from the host: reset, stats, key
    int wait_last()
    {
        XR_HIP(hipSetDevice(device));
        XR_HIP(hipStreamSynchronize(last_stream));
        return XRIT_OK;
    }
    // the host-buffer paths run on the own stream: the state's last writer is waited for if it was a foreign one
    int adopt_own_stream(hipStream_t &s)
    {
        XR_HIP(hipSetDevice(device));
        if (last_stream != stream) XR_HIP(hipStreamSynchronize(last_stream));
        s = stream;
        return XRIT_OK;
    }
    void ran_on(hipStream_t s) { last_stream = s; }
    // reset: once the last call has finished, the state becomes src's bytes (zeros without src)
    int write_state(void *dst, const void *src, size_t bytes)
    {
        XR_TRY(wait_last());
        if (src) XR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        else XR_HIP(hipMemsetAsync(dst, 0, bytes, stream));
        XR_HIP(hipStreamSynchronize(stream));
        ran_on(stream);
        return XRIT_OK;
    }
    int read_back(void *dst, const void *src, size_t bytes)
    {
        XR_TRY(wait_last());
        XR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
        XR_HIP(hipStreamSynchronize(stream));
        return XRIT_OK;
    }
};

// H derives from StageHandle and has close_all(), which hands its buffers to close()
template <class H> int stage_destroy(H *h)
{
    if (!h) return XRIT_OK;
    h->close_all();
    delete h;
    return XRIT_OK;
}

// init(H &): the stage's own allocations and start state, on the opened handle
template <class H, class Init> int stage_create(H **out, int device, Init init)
{
    if (!out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    H *h = new (std::nothrow) H;
    if (!h) { set_error("out of host memory"); return XRIT_E_NOMEM; }
    int rc = h->open(device);
    if (rc == XRIT_OK) rc = init(*h);
    if (rc != XRIT_OK) {
        stage_destroy(h);
        return rc;
    }
    *out = h;
    return XRIT_OK;
}

// One output of a host-buffer call with a capacity: the device holds min(*count, cap) elements, *count (in the summary
// the host was given) is the true number.
struct Written {
    void *dst;
    const void *src;
    size_t elem;
    const uint64_t *count;
    size_t cap;
    const char *noun;
};

// The summary, then every output's written prefix; XRIT_E_CAPACITY ("<stage>: <count> <noun>, ...: the output buffers
// are too small") when the summary says that one of them did not fit.
inline int download_written(hipStream_t s, const char *stage, void *summary, const void *d_summary, size_t summary_bytes,
                            const uint32_t *overflow, std::initializer_list<Written> outs)
{
    XR_HIP(hipMemcpyAsync(summary, d_summary, summary_bytes, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    for (const Written &w : outs) {
        const size_t n = *w.count < w.cap ? (size_t)*w.count : w.cap;
        if (n) XR_HIP(hipMemcpyAsync(w.dst, w.src, n * w.elem, hipMemcpyDeviceToHost, s));
    }
    XR_HIP(hipStreamSynchronize(s));
    if (!*overflow) return XRIT_OK;
    std::string text;
    for (const Written &w : outs) text += (text.empty() ? "" : ", ") + std::to_string(*w.count) + " " + w.noun;
    set_error("%s: %s: the output buffers are too small", stage, text.c_str());
    return XRIT_E_CAPACITY;
}

}  // namespace xrit
