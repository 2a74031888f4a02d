// framer_host_check.cpp -- the stream frame synchroniser's plain host parts (framer_host.h) in a program of their own:
// the row bound against a serial count, the argument checks, the sync words, the segment length, a call's parameters and
// the counters' copy.  Built and run
// by `make framer-host-check` with -fsanitize=address,undefined; exits non-zero on the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "framer_host.h"

using namespace xrit;
using namespace xrit::framer_host;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            return 1;                                                               \
        }                                                                           \
    } while (0)

int main()
{
    // the row bound: the worst stream for a call of n symbols consumes a frame per row from the longest carry
    for (uint32_t frame : {65u, 66u, 320u, 16384u, 1u << 20}) {
        for (size_t n : {(size_t)0, (size_t)1, (size_t)frame - 1, (size_t)frame, (size_t)frame + 1, (size_t)100000, (size_t)1 << 30}) {
            const size_t span = span_max(n, frame);
            CHECK(span == n + 2 * (size_t)frame - 66);
            CHECK(rows_cap(n, frame) == span / frame);
            CHECK(rows_cap(n, frame) * frame <= span && (rows_cap(n, frame) + 1) * frame > span);
        }
    }
    CHECK(rows_cap(0, 16384) == 1 && rows_cap(16384, 16384) == 2 && rows_cap((size_t)1 << 30, 16384) == 65537);
    CHECK(rows_cap(0, 65) == 0 && rows_cap(1, 65) == 1);

    CHECK(check_frame(16384, 46, false) == nullptr && check_frame(65, 0, false) == nullptr && check_frame(1u << 20, 64, false) == nullptr);
    CHECK(check_frame(64, 46, false) != nullptr && check_frame((1u << 20) + 1, 46, false) != nullptr);
    CHECK(check_frame(320, 65, false) != nullptr && check_frame(320, 46, true) != nullptr);

    std::vector<char> buf(16);
    const void *p = buf.data();
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p) == nullptr);
    CHECK(check_push(nullptr, p, 10, 1, p, p, p, p, p) != nullptr);
    CHECK(check_push(p, nullptr, 10, 1, p, p, p, p, p) != nullptr);
    CHECK(check_push(p, nullptr, 0, 1, p, p, p, p, p) == nullptr);              // an empty call needs no symbols
    CHECK(check_push(p, p, 0, 0, nullptr, nullptr, nullptr, nullptr, p) == nullptr);   // ... and no rows no outputs
    CHECK(check_push(p, p, 10, 1, nullptr, p, p, p, p) != nullptr && check_push(p, p, 10, 1, p, nullptr, p, p, p) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, nullptr, p, p) != nullptr && check_push(p, p, 10, 1, p, p, p, nullptr, p) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, nullptr) != nullptr);
    CHECK(check_push(p, p, XRIT_FRAMER_MAX_SYMBOLS, 1, p, p, p, p, p) == nullptr);
    CHECK(check_push(p, p, XRIT_FRAMER_MAX_SYMBOLS + 1, 1, p, p, p, p, p) != nullptr);

    // segments: the greatest power of two up to the square root, the caller's value as given, never more than 2^31 bytes
    CHECK(segment_chunks(span_max(0, 16384), 16384, 0) == 4);
    CHECK(segment_chunks((size_t)3000 * 16384, 16384, 0) == 32);
    CHECK(segment_chunks((size_t)65538 * 16384, 16384, 0) == 256);
    CHECK(segment_chunks((size_t)65535 * 16384, 16384, 0) == 128);
    CHECK(segment_chunks((size_t)1 << 30, 65, 0) == 1024);
    CHECK(segment_chunks(1000, 320, 7) == 7 && segment_chunks(1000, 320, 1) == 1);
    CHECK(segment_chunks((size_t)1 << 30, 1u << 20, 0xFFFFFFFFu) == 2048);
    for (uint32_t frame : {65u, 320u, 16384u, 1u << 20})
        for (uint32_t set : {0u, 1u, 64u, 1u << 20, 0xFFFFFFFFu})
            CHECK((uint64_t)segment_chunks(span_max((size_t)1 << 30, frame), frame, set) * frame <= ((uint64_t)1 << 31));

    // the sync words (each the other's complement on LRIT: the other phase of the lock) and a call's parameters
    uint64_t lrit[2], hrit[2];
    sync_words(0, lrit);
    sync_words(1, hrit);
    CHECK(lrit[0] == 0xfca2b63db00d9794ull && lrit[1] == 0x035d49c24ff2686bull && (lrit[0] ^ lrit[1]) == ~0ull);
    CHECK(hrit[0] == 0xfc4ef4fd0cc2df89ull && hrit[1] == 0x25010b02f33d2076ull);
    CHECK(segments(0, 16384, 4) == 1 && segments((size_t)1 << 30, 16384, 256) == 257 && segments(1, 65, 1) == 1);
    for (uint32_t frame : {65u, 320u, 16384u, 1u << 20})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)100000, (size_t)1 << 30})
            for (uint32_t set : {0u, 1u, 7u, 0xFFFFFFFFu}) {
                const FramerPar par = call_par(frame == 320, frame, 46, set, n);
                CHECK(par.frame == frame && par.min_corr == 46 && par.n == n && par.invert == (frame == 320 ? 0u : 1u));
                CHECK((((uint64_t)par.whi[0] << 32) | par.wlo[0]) == (frame == 320 ? hrit[0] : lrit[0]));
                CHECK((((uint64_t)par.whi[1] << 32) | par.wlo[1]) == (frame == 320 ? hrit[1] : lrit[1]));
                CHECK(par.cap == rows_cap(n, frame) && par.seg_chunks == segment_chunks(span_max(n, frame), frame, set));
                CHECK(par.seg_chunks >= 1 && par.seg_bytes == par.seg_chunks * frame && par.segs >= 1);
                // the segments cover the longest view, and the last one is needed for it
                CHECK((uint64_t)par.segs * par.seg_bytes >= span_max(n, frame));
                CHECK((uint64_t)(par.segs - 1) * par.seg_bytes < span_max(n, frame));
            }

    FramerState s{};
    s.symbols = 11; s.cursor = 7; s.rows = 5; s.frames = 4; s.dropped = 1; s.resyncs = 2; s.rewalked = 3; s.adopted = 2; s.calls = 9;
    s.carry = 4;
    std::vector<xrit_framer_counters> out(1);                                   // on the heap: an overrun is the sanitizer's to find
    std::memset(out.data(), 0xAB, sizeof out[0]);
    copy_counters(s, out.data());
    CHECK(out[0].symbols == 11 && out[0].cursor == 7 && out[0].rows == 5 && out[0].frames == 4 && out[0].dropped_chunks == 1);
    CHECK(out[0].resyncs == 2 && out[0].carry == 4 && out[0].rewalked_chunks == 3 && out[0].adopted_chunks == 2 && out[0].calls == 9);
    CHECK(sizeof(xrit_framer_counters) == 80);
    std::puts("framer host check ok");
    return 0;
}
