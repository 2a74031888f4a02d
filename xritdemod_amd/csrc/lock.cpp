// lock.cpp -- C ABI of the frame lock (include/xritdemod_amd.h, "Frame lock"): the handle is a SyncCore and a DecoderCore
// (frame_cores.h) -- the synchroniser's state (cursor, counters, carry) with the loop state (ok, fc) behind it, and the
// decoder's carry, in device memory -- and a mode buffer; the kernels are in lock.hip, framer.hip, viterbi.hip and
// rs.hip, the plain host parts in lock_host.h.  A call queues the bits / maxima pass and the walkers once and then rounds
// of joints, gather, decoder and commit; after every round it reads one LockRound back and goes on while the walk stopped
// for an RS outcome.
#include "frame_cores.h"

using namespace xrit;

static_assert(sizeof(xrit_lock_counters) == 136, "xrit_lock_counters: 136 bytes (LOCK_STATS_DTYPE mirrors it)");

struct xrit_lock : StageHandle {
    SyncCore sync;
    DecoderCore dec;
    uint32_t recheck = lock_host::RECHECK_DEFAULT;
    // The host's shadow of the device's `fc != 0`: a row was emitted since the reset (every consumed chunk is a row and
    // adds 1 to fc).  Set from the rounds' read-back at the end of a push that succeeded; a push that fails behind a
    // committed round leaves it false while fc is 1, and the next call then records one short hit that nothing reads.
    bool consumed = false;
    LockRound *round = nullptr;     // pinned: the record a round is read back into
    DevBuf h_mode;
    void close_all()
    {
        close();
        h_mode.release();
        sync.release();
        dec.release();
        if (round) (void)hipHostFree(round);
        round = nullptr;
    }
};

int xrit_lock_create(xrit_lock **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_lock &lk) {
        lk.sync.frame = lock_host::FRAME;
        lk.sync.min_corr = lock_host::MIN_CORRELATION;
        XR_TRY(lk.sync.open(hrit));
        XR_TRY(lk.dec.open(hrit, lk.device));
        XR_HIP(hipHostMalloc(reinterpret_cast<void **>(&lk.round), sizeof(LockRound), hipHostMallocDefault));
        return xrit_lock_reset(&lk);
    });
}

int xrit_lock_destroy(xrit_lock *lk) { return stage_destroy(lk); }

int xrit_lock_reset(xrit_lock *lk)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->consumed = false;
    XR_TRY(lk->sync.reset(*lk));
    return lk->dec.reset(*lk);
}

int xrit_lock_set_flywheel(xrit_lock *lk, uint32_t recheck)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    if (const char *why = lock_host::check_flywheel(recheck, lk->sync.started)) { set_error("%s", why); return XRIT_E_INVALID; }
    lk->recheck = recheck;
    return XRIT_OK;
}

int xrit_lock_set_segment(xrit_lock *lk, uint32_t chunks)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->sync.segment = chunks;
    return XRIT_OK;
}

int xrit_lock_set_windows(xrit_lock *lk, uint32_t windows)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->dec.set_windows(windows);
    return XRIT_OK;
}

size_t xrit_lock_rows(const xrit_lock *lk, size_t n) { return lk ? lk->sync.rows(n) : 0; }

int xrit_lock_push_device(xrit_lock *lk, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                          xrit_sync_hit *d_hits, uint64_t *d_start, uint8_t *d_mode, uint8_t *d_cadu, uint8_t *d_block,
                          xrit_frame_info *d_info, uint32_t *d_count, void *stream)
{
    constexpr uint32_t F = lock_host::FRAME;
    const size_t cap = lk ? lk->sync.rows(n) : 0;
    if (const char *why = lock_host::check_push(lk, d_symbols, n, cap, d_frames, d_valid, d_hits, d_start, d_mode, d_cadu, d_block,
                                                d_info, d_count, true)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(lk->device));
    hipStream_t s = (hipStream_t)stream;
    LockPar lp{lk->recheck, F / 16, 1, 0, lk->recheck == 1 && !lk->consumed ? 1u : 0u};
    unsigned windows = 0;
    XR_TRY(lk->dec.reserve(cap, windows));
    lk->ran_on(s);
    XR_TRY(lk->sync.begin(d_symbols, n, lp, s));
    lock_host::Rounds rounds(cap);
    for (bool again = true; again;) {
        const size_t r0 = rounds.done;                          // the gather and the decoder take the rows from r0 on
        lp.r0 = (unsigned)r0;
        XR_TRY(launch_lock_joints(lk->sync.par, lp, lk->sync.st(), lk->sync.sc, d_count, s));
        XR_TRY(lk->sync.gather(r0, d_symbols, d_frames, d_valid, d_hits, d_start, s));
        XR_TRY(lk->dec.run(d_frames + r0 * F, d_valid + r0, cap - r0, d_cadu + r0 * CADU_BYTES, d_block + r0 * BLOCK_BYTES,
                           d_info + r0, windows, s));
        XR_TRY(launch_lock_commit(lk->sync.par, lp, lk->sync.st(), lk->sync.sc, d_info, d_mode, s));
        XR_HIP(hipMemcpyAsync(lk->round, &lk->sync.st()->round, sizeof(LockRound), hipMemcpyDeviceToHost, s));
        XR_HIP(hipStreamSynchronize(s));
        if (const char *why = rounds.next(*lk->round, again)) { set_error("%s", why); return XRIT_E_HIP; }
        lp.first = 0;
    }
    lk->consumed = lk->consumed || rounds.done != 0;
    lk->sync.end();
    return XRIT_OK;
}

int xrit_lock_push(xrit_lock *lk, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                   uint64_t *start, uint8_t *mode, uint8_t *cadu, uint8_t *block, xrit_frame_info *info)
{
    const size_t cap = lk ? lk->sync.rows(n) : 0;
    uint32_t count = 0;
    if (const char *why = lock_host::check_push(lk, symbols, n, cap, frames, valid, hits, start, mode, cadu, block, info, &count, false)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    hipStream_t s;
    XR_TRY(lk->adopt_own_stream(s));
    SyncCore &y = lk->sync;
    DecoderCore &d = lk->dec;
    XR_TRY(y.upload(symbols, n, s));
    XR_TRY(lk->h_mode.reserve(cap + 4));
    XR_TRY(d.stage(cap));
    XR_TRY(xrit_lock_push_device(lk, y.h_sym.as<int8_t>(), n, y.h_frames.as<int8_t>(), y.h_valid.as<uint8_t>(),
                                 y.h_hits.as<xrit_sync_hit>(), y.h_start.as<uint64_t>(), lk->h_mode.as<uint8_t>(),
                                 d.h_cadu.as<uint8_t>(), d.h_block.as<uint8_t>(), d.h_info.as<xrit_frame_info>(),
                                 y.h_count.as<uint32_t>(), s));
    XR_TRY(y.download(n, frames, valid, hits, start, &count, s));
    if (cap) XR_HIP(hipMemcpyAsync(mode, lk->h_mode.p, cap, hipMemcpyDeviceToHost, s));
    XR_TRY(d.download(cap, cadu, block, info, s));
    XR_HIP(hipStreamSynchronize(s));
    return (int)count;
}

int xrit_lock_stats(xrit_lock *lk, xrit_lock_counters *out)
{
    if (!lk || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    LockState s;
    XR_TRY(lk->read_back(&s, lk->sync.state.p, sizeof s));
    lock_host::copy_counters(s, out);
    return XRIT_OK;
}
