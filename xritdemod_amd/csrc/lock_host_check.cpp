// lock_host_check.cpp -- the frame lock's plain host parts (lock_host.h) in a program of their own: the argument checks,
// the bookkeeping of the round loop and the counters' copy.  Built and run by `make lock-host-check` with
// -fsanitize=address,undefined; exits non-zero on the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lock_host.h"

using namespace xrit;
using namespace xrit::lock_host;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            return 1;                                                               \
        }                                                                           \
    } while (0)

int main()
{
    CHECK(FRAME == 16384 && FRAME / 16 >= 65 && MIN_CORRELATION == 46 && RECHECK_DEFAULT == 4);
    CHECK(check_flywheel(1, false) == nullptr && check_flywheel(4, false) == nullptr && check_flywheel(255, false) == nullptr);
    CHECK(check_flywheel(0, false) != nullptr && check_flywheel(256, false) != nullptr && check_flywheel(0xFFFFFFFFu, false) != nullptr);
    CHECK(check_flywheel(4, true) != nullptr);

    std::vector<char> buf(64);
    const char *base = buf.data();
    while ((size_t)base & 15) ++base;
    const void *p = base, *odd = base + 1;
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, p, p, p, p, true) == nullptr);
    CHECK(check_push(nullptr, p, 10, 1, p, p, p, p, p, p, p, p, p, true) != nullptr);
    CHECK(check_push(p, nullptr, 10, 1, p, p, p, p, p, p, p, p, p, true) != nullptr);
    CHECK(check_push(p, nullptr, 0, 1, p, p, p, p, p, p, p, p, p, true) == nullptr);               // an empty call needs no symbols
    CHECK(check_push(p, p, 10, 1, nullptr, p, p, p, p, p, p, p, p, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, nullptr, p, p, p, p, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, nullptr, p, p, p, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, p, nullptr, p, p, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, p, p, nullptr, p, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, p, p, p, nullptr, true) != nullptr);
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, odd, p, p, p, true) != nullptr);                  // the device path's cadu alignment
    CHECK(check_push(p, p, 10, 1, p, p, p, p, p, odd, p, p, p, false) == nullptr);
    CHECK(check_push(p, p, XRIT_FRAMER_MAX_SYMBOLS + 1, 1, p, p, p, p, p, p, p, p, p, true) != nullptr);
    CHECK(framer_host::rows_cap(0, FRAME) == 1);                                                   // never a call without output rows

    // the round loop: a call in lock, a call with two stops, and the records it refuses
    bool again = true;
    {
        Rounds r(5);
        CHECK(r.next(LockRound{4, 0, 65536, 0}, again) == nullptr && !again && r.done == 4 && r.rounds == 1);
    }
    {
        Rounds r(12);
        CHECK(r.next(LockRound{2, 1, 33468, 0}, again) == nullptr && again && r.done == 2);
        CHECK(r.next(LockRound{7, 1, 115388, 0}, again) == nullptr && again && r.done == 7);
        CHECK(r.next(LockRound{12, 0, 197308, 0}, again) == nullptr && !again && r.done == 12 && r.rounds == 3);
    }
    {
        Rounds r(12);
        CHECK(r.next(LockRound{13, 0, 0, 0}, again) != nullptr && !again);          // more rows than the outputs hold
        CHECK(r.next(LockRound{3, 1, 0, 0}, again) == nullptr && again);
        CHECK(r.next(LockRound{2, 0, 0, 0}, again) != nullptr && !again);           // fewer than before
        CHECK(r.next(LockRound{3, 1, 0, 0}, again) != nullptr && !again);           // a stop without a new row
        CHECK(r.next(LockRound{3, 0, 0, 0}, again) == nullptr && !again);           // ... the end of a call may add none
        CHECK(r.next(LockRound{4, 2, 0, 0}, again) != nullptr);
        CHECK(r.next(LockRound{12, 1, 0, 0}, again) != nullptr);                    // stopped with the outputs full
    }
    {
        Rounds r(0);
        CHECK(r.next(LockRound{0, 0, 0, 0}, again) == nullptr && !again);
        CHECK(r.next(LockRound{0, 1, 0, 0}, again) != nullptr);
    }

    LockState s{};
    s.fr.symbols = 11; s.fr.cursor = 7; s.fr.rows = 5; s.fr.frames = 4; s.fr.dropped = 1; s.fr.resyncs = 2; s.fr.rewalked = 3;
    s.fr.adopted = 2; s.fr.calls = 9; s.fr.carry = 4;
    s.short_kept = 21; s.short_missed = 22; s.rechecks = 23; s.sensitive = 24; s.rounds = 25; s.frames_ok = 26; s.frames_bad = 27;
    s.ok = 1; s.fc = 3;
    std::vector<xrit_lock_counters> out(1);                                     // on the heap: an overrun is the sanitizer's to find
    std::memset(out.data(), 0xAB, sizeof out[0]);
    copy_counters(s, out.data());
    CHECK(out[0].framer.symbols == 11 && out[0].framer.cursor == 7 && out[0].framer.rows == 5 && out[0].framer.frames == 4);
    CHECK(out[0].framer.dropped_chunks == 1 && out[0].framer.resyncs == 2 && out[0].framer.carry == 4 && out[0].framer.calls == 9);
    CHECK(out[0].framer.rewalked_chunks == 3 && out[0].framer.adopted_chunks == 2);
    CHECK(out[0].short_kept == 21 && out[0].short_missed == 22 && out[0].rechecks == 23 && out[0].sensitive_chunks == 24);
    CHECK(out[0].rounds == 25 && out[0].frames_ok == 26 && out[0].frames_bad == 27);
    CHECK(sizeof(xrit_lock_counters) == 136 && offsetof(LockState, fr) == 0);
    std::puts("lock host check ok");
    return 0;
}
