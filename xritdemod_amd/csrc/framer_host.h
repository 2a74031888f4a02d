// framer_host.h -- the plain host parts of the stream frame synchroniser (framer.cpp, and lock.cpp through frame_cores.h):
// the handle's state record as the kernels keep it, the sync words, the row bound, the argument checks, the segment
// length, a call's parameters and the counters' copy.  No HIP here, so that a stand-alone program can run these under a
// sanitizer on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/xritdemod_amd.h"

namespace xrit {

// the handle's state in device memory: written by the joints kernel alone, once per call
struct FramerState {
    unsigned long long symbols, cursor, rows, frames, dropped, resyncs, rewalked, adopted, calls;
    unsigned carry;                 // bytes of the stream from the cursor on, in the current carry buffer
    unsigned reserved;
};

// a call's parameters, as every kernel of the call takes them: carry ++ new symbols is the call's view V; offsets are
// relative to V[0], the cursor at the start of the call
struct FramerPar {
    unsigned frame, min_corr, invert;       // invert: LRIT (a frame found with word != 0 is inverted)
    unsigned whi[2], wlo[2];                // the two sync words
    unsigned n;                             // new symbols of this call
    unsigned seg_chunks, seg_bytes, segs;   // S, S * frame, segments (walkers) of this call
    unsigned cap;                           // rows the outputs hold
};

namespace framer_host {

constexpr uint32_t FRAME_MIN = 65, FRAME_MAX = 1u << 20;

// the two encoded 64-bit sync words the correlator is given (newdecoder.cpp:21-24)
inline void sync_words(int hrit, uint64_t words[2])
{
    words[0] = hrit ? 0xfc4ef4fd0cc2df89ull : 0xfca2b63db00d9794ull;
    words[1] = hrit ? 0x25010b02f33d2076ull : 0x035d49c24ff2686bull;
}

// rows a call of n symbols emits at most: the carry is at most 2 * frame - 66 bytes and every row consumes a frame
inline size_t rows_cap(size_t n, uint32_t frame) { return (n + 2 * (size_t)frame - 66) / frame; }

// bytes of carry ++ new symbols a call of n symbols sees at most
inline size_t span_max(size_t n, uint32_t frame) { return n + 2 * (size_t)frame - 66; }

inline const char *check_frame(uint32_t frame, uint32_t min_correlation, bool started)
{
    if (started) return "framer: frame and min_correlation are set before the first push";
    if (frame < FRAME_MIN || frame > FRAME_MAX) return "framer: 65..2^20 symbols per frame";
    if (min_correlation > 64) return "framer: min_correlation 0..64";
    return nullptr;
}

// the outputs are checked for the rows the call may write
inline const char *check_push(const void *handle, const void *symbols, size_t n, size_t rows, const void *frames,
                              const void *valid, const void *hits, const void *start, const void *count)
{
    if (!handle || !count) return "null argument";
    if (n > XRIT_FRAMER_MAX_SYMBOLS) return "framer: at most 2^30 symbols per call";
    if (n && !symbols) return "null argument";
    if (rows && (!frames || !valid || !hits || !start)) return "null argument";
    return nullptr;
}

// chunks per walker segment: `set`, or the greatest power of two whose square is at most the call's chunks (the walkers
// run S dependent queries side by side, the joints about one per segment behind one another: S + chunks / S is least
// at the square root; measured at 65536 chunks); a segment is at most 2^31 bytes
inline uint32_t segment_chunks(size_t span, uint32_t frame, uint32_t set)
{
    uint32_t s = set;
    if (!s) {
        const size_t chunks = span / frame;
        s = 4;
        while (s < 1024 && (size_t)(2 * s) * (2 * s) <= chunks) s *= 2;
    }
    const uint32_t most = (uint32_t)(((size_t)1 << 31) / frame);
    return s > most ? most : s;
}

// walker segments of S chunks that cover the longest view of a call of n symbols
inline uint32_t segments(size_t n, uint32_t frame, uint32_t seg_chunks)
{
    const size_t seg = (size_t)seg_chunks * frame;
    return (uint32_t)((span_max(n, frame) + seg - 1) / seg);
}

// the parameters of a call of n symbols; `segment` as given to segment_chunks
inline FramerPar call_par(int hrit, uint32_t frame, uint32_t min_corr, uint32_t segment, size_t n)
{
    uint64_t words[2];
    sync_words(hrit, words);
    FramerPar par{};
    par.frame = frame;
    par.min_corr = min_corr;
    par.invert = hrit ? 0u : 1u;
    for (int w = 0; w < 2; ++w) {
        par.whi[w] = (unsigned)(words[w] >> 32);
        par.wlo[w] = (unsigned)(words[w] & 0xFFFFFFFFull);
    }
    par.n = (unsigned)n;
    par.seg_chunks = segment_chunks(span_max(n, frame), frame, segment);
    par.seg_bytes = par.seg_chunks * frame;
    par.segs = segments(n, frame, par.seg_chunks);
    par.cap = (unsigned)rows_cap(n, frame);
    return par;
}

inline void copy_counters(const FramerState &s, xrit_framer_counters *out)
{
    std::memset(out, 0, sizeof *out);
    out->symbols = s.symbols;
    out->cursor = s.cursor;
    out->rows = s.rows;
    out->frames = s.frames;
    out->dropped_chunks = s.dropped;
    out->resyncs = s.resyncs;
    out->carry = s.carry;
    out->rewalked_chunks = s.rewalked;
    out->adopted_chunks = s.adopted;
    out->calls = s.calls;
}

}  // namespace framer_host
}  // namespace xrit
