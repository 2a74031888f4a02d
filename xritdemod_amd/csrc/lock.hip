// lock.hip -- the chain of the stream frame synchroniser and of the frame lock (include/xritdemod_amd.h, "Stream frame
// synchroniser", "Frame lock"; DESIGN.md sections 17 and 18): the reference decoder's walk over a stream of soft symbols,
// chunk by chunk (decoder/src/newdecoder.cpp:212-270), with its flywheel (:218-237, 321-338), where the range a chunk is
// correlated over hangs on the Reed-Solomon outcome of the frame before it.  lp.recheck == 1 is the walk without the
// flywheel: the synchroniser's, and the lock's with flywheel = 1.  The bits / maxima pass and the gather are framer.hip's,
// the decoder's kernels are viterbi.hip and rs.hip.
//
//  (b) lock_walk_kernel: V is cut into segments of S chunks; one wave per segment walks the recurrence
//      c -> c + F | c + pos + F from the segment's nominal start and records its steps.  A step is one range query over
//      positions c .. c + F - 65 (framer_query.h).  With the flywheel on, and where the whole-chunk hit is not at
//      position 0, it also records the hit over the first frame / 16 symbols.  Both are functions of the cursor alone.
//      (Where the whole-chunk hit is at position 0 the short hit equals it: the short range is a prefix of the whole, so
//      no word reaches a greater count there than in the whole, and the winner's count is reached at position 0, the
//      first of both.)
//  (c) plain_joints_kernel (the synchroniser's) and lock_joints_kernel (the lock's; without the flywheel it copies the
//      records as plain_joints_kernel does, and also writes a flag byte per row and the round's record).  The two share
//      the record search, the tally and the epilogue.  One wave follows the true chain from the cursor.  Where its cursor is a cursor the segment's
//      walker recorded, the rest of that record is the chain (the walk is a function of the cursor alone); elsewhere it
//      takes real steps until it meets the record or leaves the segment.  With the flywheel on it carries what it knows
//      of (ok, fc): ok is not known behind a valid row of this round (its RS outcome comes with the round's decoder) and
//      fc is not known behind a chunk that is MISS or FULL according to such an ok.  The hit of a chunk hangs on the
//      state only where the whole-chunk hit is not at 0 and the short one is; there the walk goes on if what it knows
//      decides the chunk and stops the round otherwise.  It writes the rows, the count, the call record and the state.
//  (e) lock_commit_kernel: behind the round's decoder, one wave replays steps 1-6 over the round's rows with their
//      info.ok: the modes, the counters and the (ok, fc) that the next round or the next call begins with.  It also
//      checks every row's hit against the one the joints chose and marks the round damaged if they differ.
//
// Without the flywheel (recheck == 1) the state changes no chunk's hit: ok = 0 and fc = 0 after a reset, fc = 1 behind
// any chunk, so step 1 fires at the entry of every later chunk and ok is 0 whenever step 2 looks at it.  Every chunk is
// FULL and a call is one round.  Only the sensitive_chunks counter then reads a short hit, and only that of the first
// chunk behind a reset (the one entered with fc != recheck): the lock's host side asks for it with lp.short0.
#include "kernels.h"
#include "framer_query.h"
#include "wave_ops.h"

namespace xrit {

namespace {

constexpr unsigned LK_NZ = 1, LK_S0 = 2, LK_USED = 4;          // FramerScratch::flags
constexpr unsigned LK_VALID = 8, LK_OK = 16;                   // ... and what the commit adds to them

// ---- what the synchroniser's chain and the lock's share ----

// the search of a walker's record for the cursor x: the index of the step recorded there, or -1
__device__ __forceinline__ int lk_find(const uint4 *__restrict__ theirs, unsigned nr, unsigned x, unsigned lane)
{
    int found = -1;
    for (unsigned base = 0; base < nr && found < 0; base += 64) {
        const unsigned idx = base + lane;
        const unsigned long long m = __ballot(idx < nr && theirs[idx].x == x);
        if (m) found = (int)(base + (unsigned)__ffsll((long long)m) - 1u);
    }
    return found;
}

// frames / dropped / resyncs of the rows a lane wrote, summed over the wave at the end
struct LkTally {
    unsigned frames = 0, dropped = 0, resyncs = 0;
    __device__ __forceinline__ void row(bool good, bool moved)
    {
        frames += good ? 1u : 0u;
        dropped += good ? 0u : 1u;
        resyncs += (good && moved) ? 1u : 0u;
    }
};

// The end of a joints kernel, by lane 0: the call record for the gather (which is given the rows from r0 on), the count
// and the framer's state; the cursor, the carry and the call are committed unless the round stopped for an RS outcome.
__device__ __forceinline__ void lk_finish(const FramerPar &par, FramerState *__restrict__ fr, unsigned L, unsigned long long T,
                                          unsigned long long x, unsigned count, unsigned count0, unsigned r0, bool stopped,
                                          const LkTally &sum, unsigned rewalked, unsigned adopted, FramerCall *__restrict__ call,
                                          unsigned *__restrict__ d_count)
{
    FramerCall cr;
    cr.base = fr->cursor;
    cr.carry = L;
    cr.total = (unsigned)T;
    cr.cursor = (unsigned)x;
    cr.count = count - r0;
    *call = cr;
    *d_count = count;
    fr->rows += count - count0;
    fr->frames += sum.frames;
    fr->dropped += sum.dropped;
    fr->resyncs += sum.resyncs;
    fr->rewalked += rewalked;
    fr->adopted += adopted;
    if (!stopped) {
        unsigned long long left = T - x;                         // at most 2 * frame - 66
        if (left > 2ull * par.frame) left = 2ull * par.frame;
        fr->symbols += par.n;
        fr->cursor += x;
        fr->calls += 1;
        fr->carry = (unsigned)left;
    }
}

__device__ __forceinline__ LkTally lk_wave_total(const LkTally &t)
{
    LkTally s;
    s.frames = wave_sum(t.frames);
    s.dropped = wave_sum(t.dropped);
    s.resyncs = wave_sum(t.resyncs);
    return s;
}

// ---- the synchroniser's joints: no flywheel, no loop state, no flags, rows as the steps ----

// (c) one wave: the true chain through the walkers' records
__global__ void __launch_bounds__(64) plain_joints_kernel(FramerPar par, FramerState *__restrict__ state,
                                                          const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax,
                                                          const uint4 *__restrict__ rec, const unsigned *__restrict__ nrec,
                                                          const uint2 *__restrict__ wout, uint4 *__restrict__ rows,
                                                          FramerCall *__restrict__ call, unsigned *__restrict__ d_count)
{
    const unsigned lane = threadIdx.x;
    const unsigned L = state->carry;
    const unsigned long long T = (unsigned long long)L + par.n;
    unsigned long long x = 0;
    unsigned count = 0, rewalked = 0, adopted = 0;
    LkTally tally;
    while (x + par.frame <= T && count < par.cap) {
        const unsigned k = (unsigned)(x / par.seg_bytes);
        if (k >= par.segs) break;
        const uint4 *theirs = rec + (size_t)k * par.seg_chunks;
        const unsigned nr = nrec[k];
        const int found = lk_find(theirs, nr, (unsigned)x, lane);
        if (found >= 0) {
            const unsigned have = nr - (unsigned)found, room = par.cap - count, m = have < room ? have : room;
            for (unsigned base = 0; base < m; base += 64) {
                const unsigned idx = base + lane;
                if (idx < m) {
                    const uint4 r = theirs[(unsigned)found + idx];
                    rows[count + idx] = r;
                    tally.row(r.w >= par.min_corr, r.z != 0);
                }
            }
            count += m;
            adopted += m;
            if (m < have) { x = theirs[(unsigned)found + m].x; break; }     // (the row bound makes this unreachable)
            const uint2 o = wout[k];
            x = o.x;
            if (o.y) break;
            continue;
        }
        const FrHit h = fr_query(par, bits, bmax, (unsigned)x, lane);
        const bool good = h.corr >= par.min_corr;
        if (good && x + h.pos + par.frame > T) break;
        if (lane == 0) {
            rows[count] = make_uint4((unsigned)x, h.word, h.pos, h.corr);
            tally.row(good, h.pos != 0);
        }
        ++count;
        ++rewalked;                                              // counted once, when the chunk is consumed
        x += good ? (unsigned long long)h.pos + par.frame : par.frame;
    }
    const LkTally sum = lk_wave_total(tally);
    if (lane == 0) lk_finish(par, state, L, T, x, count, 0u, 0u, false, sum, rewalked, adopted, call, d_count);
}

// ---- the lock's chain ----

// the hits of the chunk at c, packed as a walker's record: (c, word | short at 0 << 1 | short word << 2 |
// short count << 8, position, count).  SHORT: where the whole-chunk hit is not at 0 the short hit is asked for too
template <bool SHORT>
__device__ __forceinline__ uint4 lk_record(const FramerPar &par, const LockPar &lp, const unsigned *__restrict__ bits,
                                          const unsigned *__restrict__ bmax, unsigned c, unsigned lane)
{
    const FrHit h = fr_query(par, bits, bmax, c, lane);
    unsigned y = h.word;
    if (SHORT && h.pos != 0) {
        const FrHit hs = fr_query_span(par, bits, bmax, c, lp.span, lane);
        if (hs.pos == 0) y |= 2u | (hs.word << 2) | (hs.corr << 8);
    }
    return make_uint4(c, y, h.pos, h.corr);
}

// (b) one wave per segment; the walkers step by the whole-chunk hit.  FLY: the flywheel is on (lp.recheck > 1) and every
// step records both hits.  Without it a step is one query; the one short hit that is read then (lp.short0: that of the
// chunk at cursor 0) is added to the first walker's first record behind the walk.
template <bool FLY>
__global__ void __launch_bounds__(64) lock_walk_kernel(FramerPar par, LockPar lp, const LockState *__restrict__ state,
                                                       const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax,
                                                       uint4 *__restrict__ rec, unsigned *__restrict__ nrec, uint2 *__restrict__ wout)
{
    const unsigned k = blockIdx.x, lane = threadIdx.x;
    const unsigned long long T = (unsigned long long)state->fr.carry + par.n;
    const unsigned long long seg1 = (unsigned long long)(k + 1) * par.seg_bytes;
    unsigned long long x = (unsigned long long)k * par.seg_bytes;
    unsigned i = 0, stop = 0;
    uint4 *mine = rec + (size_t)k * par.seg_chunks;
    while (x < seg1 && i < par.seg_chunks) {
        if (x + par.frame > T) { stop = 1; break; }
        const uint4 r = lk_record<FLY>(par, lp, bits, bmax, (unsigned)x, lane);
        const bool good = r.w >= par.min_corr;
        if (good && x + r.z + par.frame > T) { stop = 1; break; }
        if (lane == 0) mine[i] = r;
        ++i;
        x += good ? (unsigned long long)r.z + par.frame : par.frame;
    }
    if (lane == 0) {
        nrec[k] = i;
        wout[k] = make_uint2((unsigned)x, stop);
    }
    if (!FLY && lp.short0 && k == 0 && i > 0) {
        const FrHit hs = fr_query_span(par, bits, bmax, 0u, lp.span, lane);
        if (lane == 0 && mine[0].z != 0 && hs.pos == 0) mine[0].y |= 2u | (hs.word << 2) | (hs.corr << 8);
    }
}

// what the joints know of the loop state.  ok: 0 false, 1 true, 2 not known in this round; fck: fc is known
struct LkTrack { unsigned ok, fc, fck; };

// the hit of a chunk: 0 the whole-chunk one, 1 the short one, 2 it hangs on something not known yet
__device__ __forceinline__ unsigned lk_decide(const LkTrack &t, unsigned R, bool nz, bool s0)
{
    if (!nz || !s0) return 0;           // position 0 under both ranges, or a short hit elsewhere: the whole-chunk hit
    if (t.ok == 0) return 0;
    if (!t.fck) return 2;
    if (t.fc == R) return 0;            // step 1 clears ok
    return t.ok == 1 ? 1 : 2;
}

// ... and the state behind the chunk, once it is consumed (steps 1, 2, 3 and 6)
__device__ __forceinline__ void lk_advance(LkTrack &t, unsigned R, bool nz, bool s0, bool valid)
{
    if (t.fck) {
        if (t.fc == R) { t.ok = 0; t.fc = 0; }
    } else if (t.ok != 0) {
        t.ok = 2;                       // step 1 may have fired
    }
    if (t.ok != 0 && nz && !s0) {       // MISS if ok holds, FULL if not: fc = 0 or fc as it was
        if (t.ok == 1) t.fc = 0;
        else t.fck = 0;
        t.ok = 0;
    }
    t.fc += 1;
    if (valid) t.ok = 2;
}

__device__ __forceinline__ unsigned lk_lane(unsigned v, unsigned i) { return (unsigned)__builtin_amdgcn_readlane((int)v, (int)i); }

// (c) one wave: the true chain through the walkers' records, from where the round before stopped.  FLY: the flywheel is
// on (lp.recheck > 1).  Without it nothing of the state is carried and no batch is stepped through, and a real step asks
// for no short hit: the one chunk whose short hit is read (lp.short0) is the call's first, which is adopted from the
// first walker's record or emits no row.
template <bool FLY>
__global__ void __launch_bounds__(64) lock_joints_kernel(FramerPar par, LockPar lp, LockState *__restrict__ state,
                                                         const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax,
                                                         const uint4 *__restrict__ rec, const unsigned *__restrict__ nrec,
                                                         const uint2 *__restrict__ wout, uint4 *__restrict__ rows,
                                                         unsigned char *__restrict__ flags, FramerCall *__restrict__ call,
                                                         unsigned *__restrict__ d_count)
{
    const unsigned lane = threadIdx.x, R = FLY ? lp.recheck : 1u;
    const unsigned L = state->fr.carry;
    const unsigned long long T = (unsigned long long)L + par.n;
    unsigned long long x = lp.first ? 0ull : (unsigned long long)state->round.cursor;
    unsigned count = lp.first ? 0u : state->round.count;
    const unsigned count0 = count;
    LkTrack t{state->ok ? 1u : 0u, state->fc, 1u};
    unsigned rewalked = 0, adopted = 0, stopped = 0;
    LkTally tally;                                          // per lane, summed at the end
    bool leave = false;
    while (!leave && x + par.frame <= T && count < par.cap) {
        const unsigned k = (unsigned)(x / par.seg_bytes);
        if (k >= par.segs) break;
        const uint4 *theirs = rec + (size_t)k * par.seg_chunks;
        const unsigned nr = nrec[k];
        const int found = lk_find(theirs, nr, (unsigned)x, lane);
        if (found < 0) {
            // a real step
            const uint4 r = lk_record<FLY>(par, lp, bits, bmax, (unsigned)x, lane);
            const bool nz = r.z != 0, s0 = FLY && (r.y & 2u) != 0;
            const unsigned d = lk_decide(t, R, nz, s0);
            if (d == 2) { stopped = 1; break; }
            const unsigned word = d ? (r.y >> 2) & 1u : r.y & 1u, pos = d ? 0u : r.z, corr = d ? r.y >> 8 : r.w;
            const bool good = corr >= par.min_corr;
            if (good && x + pos + par.frame > T) break;
            if (lane == 0) {
                rows[count] = make_uint4((unsigned)x, word, pos, corr);
                flags[count] = (unsigned char)((nz ? LK_NZ : 0u) | (s0 ? LK_S0 : 0u) | (d ? LK_USED : 0u));
                tally.row(good, pos != 0);
            }
            lk_advance(t, R, nz, s0, good);
            ++count;
            ++rewalked;                                          // counted once, when the chunk is consumed
            x += good ? (unsigned long long)pos + par.frame : par.frame;
            continue;
        }
        // the rest of the walker's record, 64 chunks at a time
        const unsigned have = nr - (unsigned)found, room = par.cap - count, m = have < room ? have : room;
        if (!FLY) {
            // the state changes no hit: the rows are the records, copied by the lanes (t is not carried through them:
            // nothing reads it behind the call's first chunk)
            for (unsigned base = 0; base < m; base += 64) {
                const unsigned idx = base + lane;
                if (idx < m) {
                    const uint4 r = theirs[(unsigned)found + idx];
                    const bool nz = r.z != 0, good = r.w >= par.min_corr;
                    rows[count + idx] = make_uint4(r.x, r.y & 1u, r.z, r.w);
                    flags[count + idx] = (unsigned char)((nz ? LK_NZ : 0u) | ((r.y & 2u) ? LK_S0 : 0u));
                    tally.row(good, nz);
                }
            }
            count += m;
            adopted += m;
        }
        bool whole = true;                                       // the record was followed to its end
        for (unsigned base = 0; FLY && base < m && whole; base += 64) {
            const unsigned idx = base + lane, cnt = m - base < 64u ? m - base : 64u;
            const bool in = idx < m;
            const uint4 r = in ? theirs[(unsigned)found + idx] : make_uint4(0, 0, 0, 0);
            const bool nz = r.z != 0, good = r.w >= par.min_corr;
            if (__ballot(in && (nz || !good)) == 0ull) {
                // in lock: every chunk a frame at position 0, whatever the state is
                if (in) {                                        // count already holds the batches before this one
                    rows[count + lane] = make_uint4(r.x, r.y & 1u, 0u, r.w);
                    flags[count + lane] = 0;
                    tally.row(true, false);
                }
                if (t.fck) {
                    const unsigned last = (t.fc + cnt - 1u) % R;             // fc at the entry of the batch's last chunk, less 1
                    t.fc = last + 1u;
                } else {
                    t.fc += cnt;
                }
                t.ok = 2;
                count += cnt;
                adopted += cnt;
                continue;
            }
            for (unsigned i = 0; i < cnt; ++i) {
                const unsigned rx = lk_lane(r.x, i), ry = lk_lane(r.y, i), rz = lk_lane(r.z, i), rw = lk_lane(r.w, i);
                const bool cnz = rz != 0, s0 = (ry & 2u) != 0;
                const unsigned d = lk_decide(t, R, cnz, s0);
                if (d == 2) {
                    stopped = 1;
                    x = rx;
                    leave = true;
                    whole = false;
                    break;
                }
                const unsigned word = d ? (ry >> 2) & 1u : ry & 1u, pos = d ? 0u : rz, corr = d ? ry >> 8 : rw;
                const bool cgood = corr >= par.min_corr;
                if (lane == 0) {
                    rows[count] = make_uint4(rx, word, pos, corr);
                    flags[count] = (unsigned char)((cnz ? LK_NZ : 0u) | (s0 ? LK_S0 : 0u) | (d ? LK_USED : 0u));
                    tally.row(cgood, pos != 0);
                }
                lk_advance(t, R, cnz, s0, cgood);
                ++count;
                ++adopted;
                if (d == 1) {                                    // position 0 kept: the chain leaves the walker's
                    x = (unsigned long long)rx + par.frame;
                    whole = false;
                    break;
                }
            }
        }
        if (!whole) continue;
        if (m < have) { x = theirs[(unsigned)found + m].x; break; }         // (the row bound makes this unreachable)
        // where the walker left; if it stopped for want of symbols, the chunk it stopped at is looked at again with
        // the lock's own hit (the short one may fit where the whole-chunk one does not)
        x = wout[k].x;
    }
    const LkTally sum = lk_wave_total(tally);
    if (lane == 0) {
        lk_finish(par, &state->fr, L, T, x, count, count0, lp.r0, stopped != 0, sum, rewalked, adopted, call, d_count);
        LockRound rd;
        rd.count = count;
        rd.stopped = stopped;
        rd.cursor = (unsigned)x;
        rd.reserved = 0;
        state->round = rd;
    }
}

// (e) one wave: steps 1-6 over the round's rows with their RS outcomes
__global__ void __launch_bounds__(64) lock_commit_kernel(FramerPar par, LockPar lp, LockState *__restrict__ state,
                                                         const uint4 *__restrict__ rows, const unsigned char *__restrict__ flags,
                                                         const xrit_frame_info *__restrict__ info, unsigned char *__restrict__ mode)
{
    const unsigned lane = threadIdx.x, R = lp.recheck;
    const unsigned count = state->round.count;
    unsigned ok = state->ok ? 1u : 0u, fc = state->fc;
    unsigned kept = 0, missed = 0, rechecks = 0, sensitive = 0, fok = 0, fbad = 0;
    unsigned differs = 0;           // rows whose hit the joints chose otherwise than the replay does
    for (unsigned base = lp.r0; base < count; base += 64) {
        const unsigned idx = base + lane, cnt = count - base < 64u ? count - base : 64u;
        const bool in = idx < count;
        unsigned sym = 0;
        if (in) {
            sym = flags[idx];
            if (rows[idx].w >= par.min_corr) sym |= LK_VALID | (info[idx].ok ? LK_OK : 0u);
        }
        unsigned mine = 0;
        if (__ballot(in && sym != (LK_VALID | LK_OK)) == 0ull) {
            // in lock, every frame good: chunk i enters with fc as below and, behind the first, with ok set
            const unsigned fci = lane == 0 ? fc : (fc + lane - 1u) % R + 1u;
            const bool rk = fci == R, oki = lane == 0 ? ok != 0 : true;
            mine = rk ? (unsigned)(XRIT_LOCK_FULL | XRIT_LOCK_RECHECK) : (oki ? XRIT_LOCK_SHORT : XRIT_LOCK_FULL);
            rechecks += (unsigned)__popcll(__ballot(in && rk));
            kept += (unsigned)__popcll(__ballot(in && mine == XRIT_LOCK_SHORT));
            fok += cnt;
            fc = (fc + cnt - 1u) % R + 1u;
            ok = 1;
        } else {
            for (unsigned i = 0; i < cnt; ++i) {
                const unsigned s = lk_lane(sym, i);
                const bool nz = (s & LK_NZ) != 0, s0 = (s & LK_S0) != 0;
                const bool rk = fc == R;
                if (rk) { ok = 0; fc = 0; ++rechecks; }
                if (!rk && nz && s0) ++sensitive;
                if (((s & LK_USED) != 0) != (ok && nz && s0)) ++differs;
                unsigned m;
                if (!ok) {
                    m = XRIT_LOCK_FULL;
                } else if (!nz || s0) {
                    m = XRIT_LOCK_SHORT;
                    ++kept;
                } else {
                    m = XRIT_LOCK_MISS;
                    ok = 0;
                    fc = 0;
                    ++missed;
                }
                ++fc;
                if (s & LK_VALID) {
                    ok = (s & LK_OK) ? 1u : 0u;
                    if (ok) ++fok; else ++fbad;
                }
                if (rk) m |= XRIT_LOCK_RECHECK;
                mine = lane == i ? m : mine;
            }
        }
        if (in) mode[idx] = (unsigned char)mine;
    }
    for (unsigned idx = count + lane; idx < par.cap; idx += 64) mode[idx] = 0;
    if (lane == 0) {
        if (differs) state->round.stopped = 2;                   // the host refuses the round (lock_host.h, Rounds::next)
        state->ok = ok;
        state->fc = fc;
        state->short_kept += kept;
        state->short_missed += missed;
        state->rechecks += rechecks;
        state->sensitive += sensitive;
        state->frames_ok += fok;
        state->frames_bad += fbad;
        state->rounds += 1;
    }
}

}  // namespace

int launch_plain_joints(const FramerPar &par, FramerState *state, FramerScratch &sc, unsigned *count, hipStream_t s)
{
    hipLaunchKernelGGL(plain_joints_kernel, dim3(1), dim3(64), 0, s, par, state, sc.bits, sc.bmax, sc.rec, sc.nrec, sc.wout, sc.rows,
                       sc.call, count);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_lock_walk(const FramerPar &par, const LockPar &lp, const LockState *state, FramerScratch &sc, hipStream_t s)
{
    const auto kernel = lp.recheck > 1 ? lock_walk_kernel<true> : lock_walk_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(par.segs), dim3(64), 0, s, par, lp, state, sc.bits, sc.bmax, sc.rec, sc.nrec,
                       sc.wout);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_lock_joints(const FramerPar &par, const LockPar &lp, LockState *state, FramerScratch &sc, unsigned *count, hipStream_t s)
{
    const auto kernel = lp.recheck > 1 ? lock_joints_kernel<true> : lock_joints_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, s, par, lp, state, sc.bits, sc.bmax, sc.rec, sc.nrec, sc.wout, sc.rows, sc.flags,
                       sc.call, count);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_lock_commit(const FramerPar &par, const LockPar &lp, LockState *state, FramerScratch &sc, const xrit_frame_info *info,
                       unsigned char *mode, hipStream_t s)
{
    hipLaunchKernelGGL(lock_commit_kernel, dim3(1), dim3(64), 0, s, par, lp, state, sc.rows, sc.flags, info, mode);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
