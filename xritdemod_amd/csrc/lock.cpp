// lock.cpp -- C ABI of the frame lock (include/xritdemod_amd.h, "Frame lock"): the handle owns the framer's state (cursor,
// counters, two carry buffers written in turn), the decoder's carry and the loop state (ok, fc) in device memory, and
// grow-only scratch; the kernels are in lock.hip, framer.hip, viterbi.hip and rs.hip, the plain host parts in
// lock_host.h.  A call queues the bits / maxima pass and the walkers once and then rounds of joints, gather, decoder and
// commit; after every round it reads one LockRound back and goes on while the walk stopped for an RS outcome.
#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_lock_counters) == 136, "xrit_lock_counters: 136 bytes (LOCK_STATS_DTYPE mirrors it)");

namespace {
constexpr unsigned LOCK_WINDOWS_PER_CU = 8;         // as the decoder's: resident Viterbi windows per CU
}  // namespace

struct xrit_lock : StageHandle {
    int hrit = 0;
    uint32_t recheck = lock_host::RECHECK_DEFAULT, segment = 0;
    unsigned slots = 0, windows = 0;
    uint64_t words[2] = {0, 0};
    bool started = false;           // a push has run: the flywheel is fixed
    int cur = 0;                    // the carry buffer the next call reads
    LockRound *round = nullptr;     // pinned: the record a round is read back into
    DevBuf state, carry[2], scratch, dcarry, prev, last, dec, verr;
    DevBuf h_sym, h_frames, h_valid, h_hits, h_start, h_mode, h_cadu, h_block, h_info, h_count;
    void close_all()
    {
        close({&state, &carry[0], &carry[1], &scratch, &dcarry, &prev, &last, &dec, &verr, &h_sym, &h_frames, &h_valid, &h_hits,
               &h_start, &h_mode, &h_cadu, &h_block, &h_info, &h_count});
        if (round) (void)hipHostFree(round);
        round = nullptr;
    }
};

int xrit_lock_create(xrit_lock **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_lock &lk) {
        int cus = 0;
        XR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, lk.device));
        lk.hrit = hrit;
        lk.slots = (unsigned)(cus > 0 ? cus : 1) * LOCK_WINDOWS_PER_CU;
        lk.windows = lk.slots;
        // newdecoder.cpp:21-24
        lk.words[0] = hrit ? 0xfc4ef4fd0cc2df89ull : 0xfca2b63db00d9794ull;
        lk.words[1] = hrit ? 0x25010b02f33d2076ull : 0x035d49c24ff2686bull;
        XR_HIP(hipHostMalloc(reinterpret_cast<void **>(&lk.round), sizeof(LockRound), hipHostMallocDefault));
        XR_TRY(lk.state.reserve(sizeof(LockState)));
        XR_TRY(lk.dcarry.reserve(64));
        XR_TRY(lk.last.reserve(sizeof(int)));
        return xrit_lock_reset(&lk);
    });
}

int xrit_lock_destroy(xrit_lock *lk) { return stage_destroy(lk); }

int xrit_lock_reset(xrit_lock *lk)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->cur = 0;
    XR_TRY(lk->write_state(lk->state.p, nullptr, sizeof(LockState)));
    return lk->write_state(lk->dcarry.p, nullptr, 64);
}

int xrit_lock_set_flywheel(xrit_lock *lk, uint32_t recheck)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    if (const char *why = lock_host::check_flywheel(recheck, lk->started)) { set_error("%s", why); return XRIT_E_INVALID; }
    lk->recheck = recheck;
    return XRIT_OK;
}

int xrit_lock_set_segment(xrit_lock *lk, uint32_t chunks)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->segment = chunks;
    return XRIT_OK;
}

int xrit_lock_set_windows(xrit_lock *lk, uint32_t windows)
{
    if (!lk) { set_error("null argument"); return XRIT_E_INVALID; }
    lk->windows = windows == 0 || windows > lk->slots ? lk->slots : windows;
    return XRIT_OK;
}

size_t xrit_lock_rows(const xrit_lock *lk, size_t n) { return lk ? framer_host::rows_cap(n, lock_host::FRAME) : 0; }

int xrit_lock_push_device(xrit_lock *lk, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                          xrit_sync_hit *d_hits, uint64_t *d_start, uint8_t *d_mode, uint8_t *d_cadu, uint8_t *d_block,
                          xrit_frame_info *d_info, uint32_t *d_count, void *stream)
{
    constexpr uint32_t F = lock_host::FRAME;
    const size_t cap = lk ? framer_host::rows_cap(n, F) : 0;
    if (const char *why = lock_host::check_push(lk, d_symbols, n, cap, d_frames, d_valid, d_hits, d_start, d_mode, d_cadu, d_block,
                                                d_info, d_count, true)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(lk->device));
    if (!lk->started) {
        for (DevBuf &c : lk->carry) XR_TRY(c.reserve(2 * (size_t)F + 16));
        lk->started = true;
    }
    FramerPar par{};
    par.frame = F;
    par.min_corr = lock_host::MIN_CORRELATION;
    par.invert = lk->hrit ? 0u : 1u;
    for (int w = 0; w < 2; ++w) {
        par.whi[w] = (unsigned)(lk->words[w] >> 32);
        par.wlo[w] = (unsigned)(lk->words[w] & 0xFFFFFFFFull);
    }
    par.n = (unsigned)n;
    par.seg_chunks = framer_host::segment_chunks(framer_host::span_max(n, F), F, lk->segment);
    par.seg_bytes = par.seg_chunks * F;
    par.segs = framer_segments(n, F, par.seg_chunks);
    par.cap = (unsigned)cap;
    LockPar lp{};
    lp.recheck = lk->recheck;
    lp.span = F / 16;
    lp.first = 1;
    lp.r0 = 0;
    LockScratch sc;
    XR_TRY(lk->scratch.reserve(lock_scratch_carve(nullptr, n, F, par.seg_chunks, sc)));
    lock_scratch_carve(lk->scratch.p, n, F, par.seg_chunks, sc);
    const unsigned windows = cap < lk->windows ? (unsigned)(cap ? cap : 1) : lk->windows;
    XR_TRY(lk->prev.reserve((cap + 1) * sizeof(int)));
    XR_TRY(lk->verr.reserve((cap + 1) * sizeof(unsigned)));
    XR_TRY(lk->dec.reserve((size_t)windows * viterbi_slot_bytes()));
    hipStream_t s = (hipStream_t)stream;
    LockState *st = lk->state.as<LockState>();
    const int8_t *carry_in = lk->carry[lk->cur].as<int8_t>();
    int8_t *carry_out = lk->carry[lk->cur ^ 1].as<int8_t>();
    lk->ran_on(s);
    XR_TRY(launch_framer_bits(par, &st->fr, carry_in, d_symbols, sc.fr, s));
    XR_TRY(launch_lock_walk(par, lp, st, sc, s));
    lock_host::Rounds rounds(cap);
    for (bool again = true; again;) {
        const size_t r0 = rounds.done, nf = cap - r0;
        lp.r0 = (unsigned)r0;
        XR_TRY(launch_lock_joints(par, lp, st, sc, d_count, s));
        FramerPar rest = par;                                   // the gather and the decoder take the rows from r0 on
        rest.cap = (unsigned)nf;
        XR_TRY(launch_framer_gather(rest, sc.fr.call, carry_in, d_symbols, sc.fr.rows + r0, carry_out, d_frames + r0 * F, d_valid + r0,
                                    d_hits + r0, reinterpret_cast<unsigned long long *>(d_start) + r0, s));
        XR_TRY(launch_viterbi(d_frames + r0 * F, d_valid + r0, nf, lk->hrit, lk->dcarry.as<int8_t>(), lk->prev.as<int>(),
                              lk->last.as<int>(), lk->dec.as<unsigned long long>(), windows, d_cadu + r0 * CADU_BYTES,
                              lk->verr.as<unsigned>(), s));
        XR_TRY(launch_rs(d_cadu + r0 * CADU_BYTES, d_valid + r0, lk->verr.as<unsigned>(), nf, d_block + r0 * BLOCK_BYTES, d_info + r0, s));
        XR_TRY(launch_lock_commit(par, lp, st, sc, d_info, d_mode, s));
        XR_HIP(hipMemcpyAsync(lk->round, &st->round, sizeof(LockRound), hipMemcpyDeviceToHost, s));
        XR_HIP(hipStreamSynchronize(s));
        if (const char *why = rounds.next(*lk->round, again)) { set_error("%s", why); return XRIT_E_HIP; }
        lp.first = 0;
    }
    lk->cur ^= 1;
    return XRIT_OK;
}

int xrit_lock_push(xrit_lock *lk, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                   uint64_t *start, uint8_t *mode, uint8_t *cadu, uint8_t *block, xrit_frame_info *info)
{
    constexpr size_t F = lock_host::FRAME;
    const size_t cap = lk ? framer_host::rows_cap(n, F) : 0;
    uint32_t count = 0;
    if (const char *why = lock_host::check_push(lk, symbols, n, cap, frames, valid, hits, start, mode, cadu, block, info, &count, false)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    hipStream_t s;
    XR_TRY(lk->adopt_own_stream(s));
    XR_TRY(lk->h_sym.reserve(n ? n : 1));
    XR_TRY(lk->h_frames.reserve(cap * F + 4));
    XR_TRY(lk->h_valid.reserve(cap + 4));
    XR_TRY(lk->h_hits.reserve((cap + 1) * sizeof(xrit_sync_hit)));
    XR_TRY(lk->h_start.reserve((cap + 1) * sizeof(uint64_t)));
    XR_TRY(lk->h_mode.reserve(cap + 4));
    XR_TRY(lk->h_cadu.reserve((cap + 1) * CADU_BYTES));
    XR_TRY(lk->h_block.reserve((cap + 1) * BLOCK_BYTES));
    XR_TRY(lk->h_info.reserve((cap + 1) * sizeof(xrit_frame_info)));
    XR_TRY(lk->h_count.reserve(sizeof(uint32_t)));
    if (n) XR_HIP(hipMemcpyAsync(lk->h_sym.p, symbols, n, hipMemcpyHostToDevice, s));
    XR_TRY(xrit_lock_push_device(lk, lk->h_sym.as<int8_t>(), n, lk->h_frames.as<int8_t>(), lk->h_valid.as<uint8_t>(),
                                 lk->h_hits.as<xrit_sync_hit>(), lk->h_start.as<uint64_t>(), lk->h_mode.as<uint8_t>(),
                                 lk->h_cadu.as<uint8_t>(), lk->h_block.as<uint8_t>(), lk->h_info.as<xrit_frame_info>(),
                                 lk->h_count.as<uint32_t>(), s));
    XR_HIP(hipMemcpyAsync(&count, lk->h_count.p, sizeof count, hipMemcpyDeviceToHost, s));
    if (cap) {
        XR_HIP(hipMemcpyAsync(frames, lk->h_frames.p, cap * F, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(valid, lk->h_valid.p, cap, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(hits, lk->h_hits.p, cap * sizeof(xrit_sync_hit), hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(start, lk->h_start.p, cap * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(mode, lk->h_mode.p, cap, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(cadu, lk->h_cadu.p, cap * CADU_BYTES, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(block, lk->h_block.p, cap * BLOCK_BYTES, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(info, lk->h_info.p, cap * sizeof(xrit_frame_info), hipMemcpyDeviceToHost, s));
    }
    XR_HIP(hipStreamSynchronize(s));
    return (int)count;
}

int xrit_lock_stats(xrit_lock *lk, xrit_lock_counters *out)
{
    if (!lk || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    LockState s;
    XR_TRY(lk->read_back(&s, lk->state.p, sizeof s));
    lock_host::copy_counters(s, out);
    return XRIT_OK;
}
