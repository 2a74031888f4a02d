// frame_cores.h -- what the three handles in front of the demultiplexer share on the host, beside stage_handle.h:
// SyncCore is the synchroniser's part of xrit_framer and xrit_lock (parameters, device state, carry, scratch, the
// launches of a call but its joints and the host-buffer staging of its four row outputs), DecoderCore the decoder's part of xrit_decoder
// and xrit_lock (resident windows, the Viterbi carry, the Viterbi + RS launches and the staging of their three outputs).
// The cores hold no stream and set no device: the handle that owns them does.  Host only.
#pragma once

#include "kernels.h"
#include "stage_handle.h"

namespace xrit {

struct SyncCore {
    int hrit = 0;
    uint32_t frame = FRAME_SYMBOLS, min_corr = 46, segment = 0;
    bool started = false;           // a push has run: what is set before the first push is fixed
    int cur = 0;                    // the carry buffer the next call reads
    DevBuf state;                   // a LockState; the synchroniser uses the FramerState in front of it
    DevBuf carry[2], scratch;       // two carry buffers, written in turn
    DevBuf h_sym, h_frames, h_valid, h_hits, h_start, h_count;
    FramerPar par{};                // of the call in progress
    FramerScratch sc{};

    int open(int hrit_)
    {
        hrit = hrit_;
        return state.reserve(sizeof(LockState));
    }
    void release()
    {
        for (DevBuf *b : {&state, &carry[0], &carry[1], &scratch, &h_sym, &h_frames, &h_valid, &h_hits, &h_start, &h_count}) b->release();
    }
    int reset(StageHandle &h)
    {
        cur = 0;
        return h.write_state(state.p, nullptr, sizeof(LockState));
    }
    size_t rows(size_t n) const { return framer_host::rows_cap(n, frame); }
    LockState *st() const { return state.as<LockState>(); }

    // The head of a call of n symbols: its parameters, the carry buffers at the first push, the scratch, then the
    // bits / maxima pass and the walkers.
    int begin(const int8_t *d_symbols, size_t n, const LockPar &lp, hipStream_t s)
    {
        if (!started) {
            for (DevBuf &c : carry) XR_TRY(c.reserve(2 * (size_t)frame + 16));
            started = true;
        }
        par = framer_host::call_par(hrit, frame, min_corr, segment, n);
        XR_TRY(scratch.reserve(framer_scratch_carve(nullptr, n, frame, par.seg_chunks, sc)));
        framer_scratch_carve(scratch.p, n, frame, par.seg_chunks, sc);
        XR_TRY(launch_framer_bits(par, &st()->fr, carry[cur].as<int8_t>(), d_symbols, sc, s));
        return launch_lock_walk(par, lp, st(), sc, s);
    }
    // Behind a round's joints: the gather of the rows from r0 to the outputs' end and of the next call's carry.  The
    // synchroniser's call is one round with r0 = 0; the output pointers are the call's.
    int gather(size_t r0, const int8_t *d_symbols, int8_t *d_frames, uint8_t *d_valid, xrit_sync_hit *d_hits, uint64_t *d_start,
               hipStream_t s)
    {
        FramerPar rest = par;
        rest.cap = par.cap - (unsigned)r0;
        return launch_framer_gather(rest, sc.call, carry[cur].as<int8_t>(), d_symbols, sc.rows + r0, carry[cur ^ 1].as<int8_t>(),
                                    d_frames + r0 * frame, d_valid + r0, d_hits + r0,
                                    reinterpret_cast<unsigned long long *>(d_start) + r0, s);
    }
    void end() { cur ^= 1; }

    // the host-buffer path: the staging buffers of a call of n symbols and the upload of the symbols ...
    int upload(const int8_t *symbols, size_t n, hipStream_t s)
    {
        const size_t cap = rows(n);
        XR_TRY(h_sym.reserve(n ? n : 1));
        XR_TRY(h_frames.reserve(cap * frame + 4));
        XR_TRY(h_valid.reserve(cap + 4));
        XR_TRY(h_hits.reserve((cap + 1) * sizeof(xrit_sync_hit)));
        XR_TRY(h_start.reserve((cap + 1) * sizeof(uint64_t)));
        XR_TRY(h_count.reserve(sizeof(uint32_t)));
        if (n) XR_HIP(hipMemcpyAsync(h_sym.p, symbols, n, hipMemcpyHostToDevice, s));
        return XRIT_OK;
    }
    // ... and the download of the count and the four row outputs, queued on s (the caller waits)
    int download(size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits, uint64_t *start, uint32_t *count, hipStream_t s)
    {
        const size_t cap = rows(n);
        XR_HIP(hipMemcpyAsync(count, h_count.p, sizeof *count, hipMemcpyDeviceToHost, s));
        if (!cap) return XRIT_OK;
        XR_HIP(hipMemcpyAsync(frames, h_frames.p, cap * frame, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(valid, h_valid.p, cap, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(hits, h_hits.p, cap * sizeof(xrit_sync_hit), hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(start, h_start.p, cap * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        return XRIT_OK;
    }
};

struct DecoderCore {
    static constexpr unsigned WINDOWS_PER_CU = 8;   // resident Viterbi windows per CU: decision scratch of 66 KB each
    int hrit = 0;
    unsigned slots = 0;             // resident windows: CUs x WINDOWS_PER_CU
    unsigned windows = 0;           // ... of which a call uses at most this many (set_windows)
    DevBuf carry;                   // the reference's lastFrameEnd (newdecoder.cpp:141,274,300)
    DevBuf prev, last, dec, verr;
    DevBuf h_cadu, h_block, h_info;

    int open(int hrit_, int device)
    {
        int cus = 0;
        XR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        hrit = hrit_;
        slots = (unsigned)(cus > 0 ? cus : 1) * WINDOWS_PER_CU;
        windows = slots;
        XR_TRY(carry.reserve(64));
        return last.reserve(sizeof(int));
    }
    void release()
    {
        for (DevBuf *b : {&carry, &prev, &last, &dec, &verr, &h_cadu, &h_block, &h_info}) b->release();
    }
    int reset(StageHandle &h) { return h.write_state(carry.p, nullptr, 64); }
    void set_windows(uint32_t w) { windows = w == 0 || w > slots ? slots : w; }

    // scratch for runs of up to nf rows; use: the resident windows such a run takes
    int reserve(size_t nf, unsigned &use)
    {
        const size_t rows = nf ? nf : 1;
        use = rows < windows ? (unsigned)rows : windows;
        XR_TRY(prev.reserve(rows * sizeof(int)));
        XR_TRY(verr.reserve(rows * sizeof(unsigned)));
        return dec.reserve((size_t)use * viterbi_slot_bytes());
    }
    // Viterbi behind the carry in `use` resident windows (as reserve gave them), then derandomiser and RS, over nf rows
    int run(const int8_t *d_frames, const uint8_t *d_valid, size_t nf, uint8_t *d_cadu, uint8_t *d_block, xrit_frame_info *d_info,
            unsigned use, hipStream_t s)
    {
        XR_TRY(launch_viterbi(d_frames, d_valid, nf, hrit, carry.as<int8_t>(), prev.as<int>(), last.as<int>(),
                              dec.as<unsigned long long>(), use, d_cadu, verr.as<unsigned>(), s));
        return launch_rs(d_cadu, d_valid, verr.as<unsigned>(), nf, d_block, d_info, s);
    }

    // the host-buffer path: the staging buffers of nf rows, and their download queued on s (the caller waits)
    int stage(size_t nf)
    {
        XR_TRY(h_cadu.reserve((nf + 1) * CADU_BYTES));
        XR_TRY(h_block.reserve((nf + 1) * BLOCK_BYTES));
        return h_info.reserve((nf + 1) * sizeof(xrit_frame_info));
    }
    int download(size_t nf, uint8_t *cadu, uint8_t *block, xrit_frame_info *info, hipStream_t s)
    {
        if (!nf) return XRIT_OK;
        XR_HIP(hipMemcpyAsync(cadu, h_cadu.p, nf * CADU_BYTES, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(block, h_block.p, nf * BLOCK_BYTES, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(info, h_info.p, nf * sizeof(xrit_frame_info), hipMemcpyDeviceToHost, s));
        return XRIT_OK;
    }
};

}  // namespace xrit
