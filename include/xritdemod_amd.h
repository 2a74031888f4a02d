/*
 * xritdemod_amd.h -- C ABI of the MI355X-native xRIT BPSK demodulation chain.
 *
 * The reference (opensatelliteproject/xritdemod) has no FFI for this path; the
 * seam is the libSatHelper C++ class API as used by
 * demodulator/src/demodulator.cpp.  Every entry point below names the
 * reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - plain C: opaque handles, pointers and sizes; no exceptions cross the ABI.
 *   - return value: 0 (XRIT_OK) or a negative XRIT_E_* code; xrit_last_error()
 *     gives the text of the last failure on the calling thread.
 *   - complex samples are interleaved (re, im) float32 = std::complex<float>.
 *   - "host" entry points take host pointers and do the H2D/D2H copies;
 *     "_device" entry points take device pointers (HBM-resident data) and a
 *     hipStream_t passed as void* (NULL = the handle's own stream).
 *   - a handle is single-consumer (the reference calls Work() from one thread,
 *     demodulator.cpp:170-175,475); distinct handles may be used concurrently.
 *   - the compute path is HIP only: if no HIP device is usable, create fails
 *     with XRIT_E_NO_DEVICE.  There is no CPU fallback.
 */
#ifndef XRITDEMOD_AMD_H_
#define XRITDEMOD_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XRIT_OK            0
#define XRIT_E_INVALID    -1   /* bad argument */
#define XRIT_E_NO_DEVICE  -2   /* no usable HIP device */
#define XRIT_E_HIP        -3   /* HIP runtime error (text in xrit_last_error) */
#define XRIT_E_NOMEM      -4
#define XRIT_E_CAPACITY   -5   /* output buffer too small */
#define XRIT_E_NOT_CONVERGED -6 /* strict mode only: hand-off passes exhausted */

/* FrontendDevice.h:11-13 */
#define XRIT_SAMPLE_FLOATIQ 0
#define XRIT_SAMPLE_S16IQ   1
#define XRIT_SAMPLE_S8IQ    2
/* not a FrontendDevice.h type: the RTL-SDR frontend converts its unsigned bytes itself and hands floats to
 * onSamplesAvailable (RtlFrontend.cpp:102-116: lut[b] = (b - 128) / 127.f, then a running-average DC tracker with
 * alpha = 1 - exp(-1 / (0.05 sampleRate)), :57).  With this type the chain takes the raw bytes and does that
 * conversion on the device, statement for statement (including the reference's `i % 1`, which makes one average
 * serve I and Q alike). */
#define XRIT_SAMPLE_U8IQ    3

const char *xrit_last_error(void);
const char *xrit_version(void);
/* number of visible HIP devices (0 when none / runtime unusable) */
int xrit_device_count(void);
/* 1 when the library was built with the measurement switches of DESIGN.md section 7 (make EXTRA=-DXRIT_EXPERIMENTS: the
 * matrix-pipe decimator, walker teams, A/B environment switches); the shipped build has none of them: 0 */
int xrit_build_experiments(void);

/* ------------------------------------------------------------------------
 * Tap designers -- SatHelper::Filters (demodulator.cpp:443-444), host only.
 * ------------------------------------------------------------------------ */
/* Filters::lowPass(gain, sampleRate, cutFreq, transitionWidth, HAMMING, beta)
 * -> number of taps written, or the negative required count if cap is short */
int xrit_lowpass_taps(double gain, double sample_rate, double cutoff, double transition_width,
                      float *taps, int cap);
/* Filters::RRC(gain, sampleRate, symbolRate, alpha, nTaps) -> taps written */
int xrit_rrc_taps(double gain, double sample_rate, double symbol_rate, double alpha, int ntaps,
                  float *taps, int cap);
/* the 129 x 8 MMSE interpolator table used by ClockRecovery */
void xrit_mmse_table(float *table /* [129*8] */);

/* ------------------------------------------------------------------------
 * The chain -- processSamples(), demodulator.cpp:100-168, with the objects
 * main() builds at demodulator.cpp:436-450.
 * ------------------------------------------------------------------------ */
typedef struct xrit_demod xrit_demod;

typedef struct xrit_demod_config {
    /* reference parameters */
    float    sample_rate;       /* device->GetSampleRate(), demodulator.cpp:436 */
    uint32_t decimation;        /* baseDecimation, cfg "decimation" (:300-301) */
    uint32_t symbol_rate;       /* cfg "symbolRate"; LRIT 293883 / HRIT 927000 */
    float    rrc_alpha;         /* cfg "rrcAlpha"; 0.5 / 0.3 */
    int32_t  rrc_taps;          /* RRC_TAPS = 63, Parameters.h:28 */
    float    agc_rate, agc_reference, agc_gain, agc_max_gain;   /* Parameters.h:34-37 */
    float    pll_alpha;         /* Costas loop bandwidth = CLOCK_ALPHA (demodulator.cpp:220) */
    float    clock_mu, clock_alpha, clock_gain_omega, clock_omega_limit; /* Parameters.h:30-33 */
    /* placement */
    int32_t  device;            /* HIP device ordinal */
    /* time-slice tiling of the feedback loops (0 = library default) */
    int32_t  costas_chain_len;  /* samples per Costas chain: 0 = 256, else 16..320 (rejected beyond: a chain that is
                                 * long against the loop's pull-in time ends in a state that is no longer a smooth
                                 * function of its start, and the hand-off solve then needs tens of passes or does
                                 * not close -- fuzz, HRIT at 512: 186 passes and flipped decisions) */
    int32_t  clock_chain_syms;  /* symbols per clock-recovery chain; 0 = chosen per call (64..256) so that the call's
                                 * waves fill whole generations of what the chip holds.  Every chain boundary is a
                                 * place where the recovered clock may differ from the serial loop's by the loop's
                                 * own chaos level, so short chains cost parity; values below
                                 * 32 are raised to 32 (16-symbol chains measured 6.5e-4 rms against 2.2e-4 at
                                 * the default and were seen to mis-resolve a symbol slip at Es/N0 < 4 dB) */
    int32_t  max_passes;        /* hand-off passes before giving up (per loop); 0 = 192: a locked signal needs 2 + 5,
                                 * a cold start within the loops' lock-in range ~15, a pull-in with cycle slips
                                 * a pass or two per chain of the slipping stretch */
    int32_t  strict;            /* 1: XRIT_E_NOT_CONVERGED when the Costas hand-off stays above its tolerance or the
                                 * clock hand-off ends with large residuals / open slips (stats.clock_open_large) */
    int32_t  clock_min_passes;  /* clock hand-off passes always run (0 = default); max_passes caps both loops */
    int32_t  slices;            /* ignored (round 1 could cut a call into time slices on two streams; measured slower
                                   on MI355X and removed) */
    int32_t  clock_serial;      /* 1: the clock recovery runs as ONE serial trajectory on the device (a single wave,
                                 * ~0.3 us per symbol) instead of time-tiled chains: no hand-offs, so what is left
                                 * against the CPU chain is what any float32 M&M fed by this chain's Costas output
                                 * shows (the recurrence lives on a 2^-21-sample lattice and keeps a one-ulp
                                 * difference for ~1e5 symbols).  A diagnostic, not a production mode. */
    int32_t  clock_exact;       /* the relay of the clock recovery (csrc/clock_relay.h): the call is cut into segments that
                                 * are walked with the literal recurrence, 64 symbols per step, from the end states the
                                 * segments in front of them reached a pass earlier.  Every pass extends what a segment
                                 * knows of its past by one segment (no shorter than 16 384 symbols unless the relay
                                 * runs to closure); a pass that changes nothing has reproduced the serial trajectory
                                 * (clock_serial = 1) bit for bit.
                                 *   0 (default), by call size (round 4): up to 74 k symbols (200 k where the call takes the bit-exact front end: cfg.front_exact 0 / 2) ONE exact walk from the carried
                                 *      state (the serial trajectory itself); from 6 M symbols -- every BASELINE burst -- no hand-off
                                 *      passes at all: two walkers per CU, the first relay pass from the timing guess, three passes at
                                 *      24.8 k symbols per segment, two from 49 k (soft symbols 5.6e-5 rms from the serial
                                 *      trajectory, within 5 % of its own distance from the CPU chain; 2.1 ms per streamed 256 Mi-sample
                                 *      burst); in between two hand-off passes, then three relay passes.  Walked to closure on its own
                                 *      when the soft symbols of the first relay pass show Es/N0 below 7 dB (hard decisions
                                 *      would otherwise differ from the serial loop's), when a segment start moves by a quarter of
                                 *      a symbol between passes (the guess miscounted) or the hand-off passes never closed,
                                 *      and four passes at a time while the segment starts still move by more than 6e-4
                                 *      sample rms from pass to pass (stats.clock_relay_passes / clock_relay_closed);
                                 *   1: every call to closure (~9 ms per 256 Mi-sample burst; the serial wave: 3.9 s);
                                 *   n > 1: two hand-off passes and n relay passes, nothing else;
                                 *   -2: hand-off passes only, five of them on a clean signal -- the fast configuration
                                 *      (2.1 ms per burst, soft symbols 2.2e-4 .. 2.6e-4 rms from the serial trajectory:
                                 *      DESIGN.md section 6); a call whose passes stall above 3e-4 sample rms (low Es/N0)
                                 *      or never close is still relayed to closure (rounds 2-3's default);
                                 *   -1: hand-off passes only, never relayed;
                                 *   -3: the quick relay -- the default's plan with the passes in front of its last walked
                                 *      approximately (one guess round, then two; no literal verification, nothing stored: they are
                                 *      there for their end states): 1.92 ms per streamed burst, 1.15e-4 rms from the serial
                                 *      trajectory.  Faster AND closer than -2. */
    int32_t  clock_exact_window;/* chains per relay segment; 0 = chosen per call (~4 segments per CU) */
    int32_t  front_exact;       /* which front end a call takes (round 6).  0 (default): the bit-exact one (see 2) on calls below the
                                 * big-burst size -- the reference's chunk sizes and everything up to a million symbols, where a call
                                 * is launch latency, not throughput: a call of up to 200 k symbols (every chunk the reference hands its blocks, 512 Ki
                                 * samples = 123 k symbols LRIT / 194 k HRIT included) is ONE exact walk of the clock recovery and yields the CPU chain's soft
                                 * symbols word for word -- and the fast one on bursts of a million symbols and more (what `value`
                                 * is quoted on); -1: the fast one on calls of every size (round 5's default).
                                 * The fast front end:  What the soft symbols' distance from the CPU chain is made
                                 * of is the front end's distance at the Costas loop's output (1.1e-6 rms as shipped; ANY distance
                                 * costs a float32 M&M 5.5e-5 on LRIT), and most of that is what the
                                 * hand-offs between the loop's 256-sample chains leave: a chain's start a few 1e-6 rad beside its
                                 * predecessor's end (a chain walked again from a start an ulp away rounds its 256 steps afresh: more passes do not
                                 * remove it), which
                                 * the loop forgets at a half per ~600 samples.
                                 *   1: the Costas loop's final pass starts every chain FOUR chains early and walks those samples
                                 *      quietly -- the stage's distance from the serial loop 1.16e-6 -> 6.1e-7, the soft symbols on
                                 *      steady-state 256 Mi-sample LRIT bursts 9.8e-5 -> 8.4e-5 rms (five bursts; HRIT 1.33e-4 ->
                                 *      1.20e-4: still a miss), for 12 % of such a burst's time (3-5 % at decimation 32; 20-30 % without a decimator, where the
                                 *      circuit-rate stream is the whole burst: profiles/r5_costas_variants_parity.json, r5_bench_c*.json).
                                 *   2 (round 6): the front end BIT FOR BIT the CPU chain's through the Costas loop -- both filters
                                 *      summed in the CPU chain's order without FMA (fir.hip: fir_exact_kernel), the AGC walked
                                 *      literally in warmed-up chains (agc.hip), the Costas loop walked exactly 64 samples per
                                 *      step with the C library's sincosf evaluated in double precision (costas_exact.hip).
                                 *      What is left of the soft symbols' distance is the clock recovery's own (its distance
                                 *      from the serial trajectory, 5-6e-5 LRIT) -- and on calls of up to 200 k symbols nothing: in
                                 *      this mode, as in the default, such a call's clock recovery is ONE exact walk from the carried state
                                 *      (with the fast front end on calls of every size, -1 / 1: up to 74 k), so every chunk the reference hands its blocks --
                                 *      32 Ki .. 512 Ki samples, at most 123 k symbols LRIT / 194 k HRIT, demodulator.cpp:108-119 --
                                 *      comes out as the CPU chain's soft symbols word for word (a 512 Ki-sample call: 5.0 ms
                                 *      instead of 3.2). */
    int32_t  reserved[2];
} xrit_demod_config;

/* setLRITMode / setHRITMode + Parameters.h defaults (demodulator.cpp:177-197) */
void xrit_demod_config_lrit(xrit_demod_config *cfg, float sample_rate, uint32_t decimation);
void xrit_demod_config_hrit(xrit_demod_config *cfg, float sample_rate, uint32_t decimation);

int  xrit_demod_create(const xrit_demod_config *cfg, xrit_demod **out);
void xrit_demod_destroy(xrit_demod *d);

/* One processSamples() pass: onSamplesAvailable conversion (:54-74), decimator
 * (:136-140, n/decimation outputs, remainder dropped), AGC (:143), RRC (:148),
 * Costas (:152), clock recovery (:156); soft_out receives Re(symbol)
 * (SymbolManager.cpp:104).  State persists across calls like the SatHelper
 * objects.  cap must be >= n/(decimation*sps*0.99)+64: a smaller one is refused before anything runs
 * (XRIT_E_CAPACITY, n_out = a capacity that suffices, the handle unchanged).  A call that fails later, after a
 * stage has advanced its carried state, leaves the handle unusable (every further call returns XRIT_E_INVALID).
 * Host buffers. */
int xrit_demod_process(xrit_demod *d, const void *samples, size_t n_complex, int sample_type,
                       float *soft_out, size_t cap, size_t *n_out);
/* Same with device-resident input and output (no PCIe in the call). */
int xrit_demod_process_device(xrit_demod *d, const void *d_samples, size_t n_complex, int sample_type,
                              float *d_soft_out, size_t cap, size_t *n_out, void *stream);
/* The clock recovery of the LAST process call once more, on the sign-flipped Costas output (xrit_group_*: this
 * rank's Costas loop locked pi away from the stream the capture's first GPU follows; the Mueller & Mueller detector
 * slices to {0, 1}, so the loop on -y is not minus the loop on y and the recovery has to run on the right sign).
 * The clock recovery's carried state goes back to what it was before that call (history and unread tail change sign),
 * the Costas loop's carried phase moves by pi; d_soft receives the call's symbols again.
 * Refused (XRIT_E_INVALID, nothing changed) while an input registered with xrit_demod_prefetch_device waits for its
 * process call: its front end and Costas loop may already have started from the unflipped state. */
int xrit_demod_redo_clock_flipped(xrit_demod *d, float *d_soft_out, size_t cap, size_t *n_out, void *stream);
/* Called after the process call that warmed the chain up over a time slice's halo (from a cold start): that call's
 * clock recovery is run once more on the negated Costas output and what it would carry is kept aside, so that a later
 * xrit_demod_redo_clock_flipped starts from the flipped loop's own state (without it, it starts from this sign's state
 * with the symbol history negated -- right to 1e-3 sample in timing, which takes 1e4..1e5 symbols to settle).
 * Refused like xrit_demod_redo_clock_flipped while a prefetched input waits. */
int xrit_demod_prepare_flipped(xrit_demod *d, void *stream);
/* Move the carried Costas phase by pi (a freshly reset chain: 0 -> pi).  The loop's equations do not see a half turn
 * (the BPSK detector I*Q does not), so a chain started so pulls in along the same path into the other of its two locks:
 * how a rank of xrit_group_* that found itself pi away from the stream starts again with the bit-exact front end, to
 * meet the stream's own float32 trajectory instead of its negative-to-rounding.  (The reference starts at 0 and keeps
 * whichever lock it falls into, demodulator.cpp:152.)  Refused while a prefetched input waits. */
int xrit_demod_flip_costas_phase(xrit_demod *d, void *stream);
/* The clock recovery's carried state as one device record of xrit_demod_clock_carry_bytes() bytes (the Mueller & Mueller
 * loop's mu, omega, last symbols and decisions, and the <= 1024 de-rotated samples it has not consumed yet):
 * which = 0: what the NEXT process call starts from, which = 1: what the LAST one started from.  The reference's loop
 * objects carry ONE state across all chunks (demodulator.cpp:446-450, 136-157); across the GPUs of xrit_group_* this record
 * is that state, handed from the rank in front to the rank behind. */
size_t xrit_demod_clock_carry_bytes(void);
int xrit_demod_export_clock_carry(xrit_demod *d, int which, void *d_record, void *stream);
/* The clock recovery of the LAST process call once more from another handle's record (which = 0 of the handle that
 * demodulated the samples in front): same input, that loop state in front of it; d_soft receives the call's symbols again.
 * Refused (XRIT_E_INVALID, nothing changed) while a prefetched input waits, or for a record that is not one. */
int xrit_demod_redo_clock_from(xrit_demod *d, const void *d_record, float *d_soft_out, size_t cap, size_t *n_out, void *stream);
/* 1 if the last process call's symbols are those of ONE float32 walk from the state it started from (cfg.clock_serial,
 * the exact closure cfg.clock_exact = 1, or a call short enough for a single exact walk -- up to 200 k symbols in the
 * default configuration and with cfg.front_exact = 2, 73 k with the fast front end on calls of every size), 0 if they are relayed / overlapping walks (close to it, not it), < 0 on a null handle. */
int xrit_demod_last_clock_exact(const xrit_demod *d);
/* 1 if a process call of n_complex input samples on this handle takes the bit-exact front end (cfg.front_exact and the
 * call's length decide, see xrit_demod_config), 0 if the fast one, < 0 on a null handle. */
int xrit_demod_front_exact_for(const xrit_demod *d, size_t n_complex);
/* Streaming at full rate: register the input of a LATER process call now, so that the library can run it ahead of
 * that call on streams of its own while the calls in between are at work:
 *     prefetch(b); prefetch(b+1);  prefetch(b+2); process_device(b);  prefetch(b+3); process_device(b+1);  ...
 * Inputs are taken by the process calls in the order they were registered (each must pass exactly the registered
 * pointer, count and type) and must stay valid until the call that takes them has returned.  The reference's input FIFO
 * plays the same role (demodulator.cpp:38,54-74: the frontend thread fills it while the DSP thread works).  A no-op while
 * stage copies or full per-kernel profiling are on.  What runs ahead, and how many inputs may wait:
 *   * calls of a million symbols or more in the default configuration (round 5: the clock recovery walks overlapping
 *     blocks, csrc/clock_overlap.h, and waits for no other burst): the front end, the Costas loop AND the clock
 *     recovery's walkers of the next TWO bursts -- three inputs may wait (the call in progress and two behind it).  A
 *     process call enqueues what the newest registration allows, waits for its own walkers and lays out its symbols;
 *   * every other call (smaller calls, clock_exact != 0): the front end and the Costas loop of the NEXT burst, started in
 *     front of the current call's relay kernels (round 4) or at once (clock_exact < 0) -- two inputs may wait.
 * The symbols are those of plain consecutive calls, word for word, either way.  XRIT_E_INVALID when as many inputs as
 * may wait are waiting already. */
int xrit_demod_prefetch_device(xrit_demod *d, const void *d_samples, size_t n_complex, int sample_type, void *stream);
/* How many inputs of n_complex samples may wait BEHIND the call in progress on this handle: 2 (calls that walk overlapping
 * blocks), 1 (every other call), 0 (stage copies or full profiling are on: nothing runs ahead). */
int xrit_demod_prefetch_depth(xrit_demod *d, size_t n_complex);
/* Back to the state right after xrit_demod_create (filter histories, gain, loop states, unread tail), without
 * giving up the device buffers: the start of another stream.  Also revives a handle a failed call left unusable. */
int xrit_demod_reset(xrit_demod *d, void *stream);
/* the hipStream_t the handle runs on when a call passes stream = NULL */
void *xrit_demod_stream(xrit_demod *d);
/* symbols per sample as the reference computes it (demodulator.cpp:437) */
float xrit_demod_sps(const xrit_demod *d);
int   xrit_demod_decimator_ntaps(const xrit_demod *d);

/* Diagnostics: enable=1 makes every later process call keep a copy of each
 * stage's output (costs D2D copies and un-fuses the stages; off by default).
 * enable=2 keeps only stage 4, the complex symbols that DiagManager::addSamples
 * taps (demodulator.cpp:161-163), at no other cost. */
int xrit_demod_keep_stages(xrit_demod *d, int enable);
/* Copies a stage's output of the LAST process call to host (tests/diagnostics):
 * 0 decimator, 1 agc, 2 rrc, 3 costas, 4 clock recovery (complex symbols).
 * Returns the element count through n; out may be NULL to query the count. */
int xrit_demod_read_stage(xrit_demod *d, int stage, float *out_interleaved, size_t cap, size_t *n);

typedef struct xrit_demod_stats {
    uint64_t samples_in;          /* last call */
    uint64_t circuit_samples;
    uint64_t symbols_out;
    int32_t  costas_passes;       /* hand-off passes run, last call */
    int32_t  clock_passes;
    uint32_t costas_unconverged;  /* chain boundaries left above tolerance */
    uint32_t clock_unconverged;   /* boundaries the last clock hand-off solve still moved: close to all of them on any
                                   * healthy call (they keep moving at the recurrence's own 1e-4 floor), NOT a failure
                                   * count -- that is clock_open_large */
    float    costas_max_residual; /* rad */
    float    clock_max_residual;  /* samples */
    int32_t  agc_serial_fallback; /* 1 if the affine scan guard tripped (|x|*rate > 1) */
    uint32_t clock_open_large;    /* boundaries left with a timing residual beyond 0.02 sample or an unresolved symbol
                                   * slip when the passes ended: 0 on a healthy call; non-zero means acquisition did
                                   * not finish within max_passes (symbol count or decisions may be off) */
    int32_t  costas_serial_walk;  /* 1 if the carrier hand-off was still open after 32 passes (pull-in through cycle
                                   * slips closes a chain or two per pass) and the open region was walked by one
                                   * serial wave instead: exact, ~0.1 us per sample of the region, once per acquisition */
    int32_t  clock_relay_passes;  /* clock_exact: relay passes of the last call (the closing one included) */
    int32_t  clock_relay_closed;  /* ... 1 if they ended with a pass that changed nothing: the symbols are the serial
                                   * trajectory's, bit for bit */
    int32_t  clock_relay_segments;/* ... segments the call was cut into */
} xrit_demod_stats;
int xrit_demod_get_stats(const xrit_demod *d, xrit_demod_stats *s);

/* Per-kernel timing with HIP events on the stream the kernels are launched on.
 * enable=1 brackets every launch of the following process calls; enable=2 only the decimating FIR (the
 * launch that reads the input) -- an event record is a queue barrier that stops neighbouring kernels from
 * overlapping, about 0.27 ms per 256 Mi-sample burst when all ~70 launches are bracketed; enable=0: off. */
int xrit_demod_profile(xrit_demod *d, int enable);
/* name/ms arrays are filled with up to cap entries (accumulated since enable);
 * launches[] = number of launches per kernel.  Returns entries written. */
int xrit_demod_profile_read(xrit_demod *d, const char **names, float *total_ms, int *launches, int cap);
/* every bracket of one kernel name since enable, in launch order (min / median of a kernel, not only its mean);
 * returns the number written */
int xrit_demod_profile_samples(xrit_demod *d, const char *name, float *ms, int cap);

/* SymbolManager::process quantiser (SymbolManager.cpp:43-46): f=s*127, clamp
 * [-128,127], C cast (truncation).  Device kernel on device pointers. */
int xrit_quantize_i8_device(const float *d_soft, int8_t *d_out, size_t n, int device, void *stream);
int xrit_quantize_i8(xrit_demod *d, const float *soft, int8_t *out, size_t n);

/* ------------------------------------------------------------------------
 * Decoder front end ("next" row): frame synchronisation.
 * Replaces SatHelper::Correlator as decoder/src/newdecoder.cpp uses it before
 * Viterbi: addWord() of the encoded 64-bit sync words (:145-151; LRIT
 * 0xfca2b63db00d9794 / 0x035d49c24ff2686b, HRIT 0xfc4ef4fd0cc2df89 /
 * 0x25010b02f33d2076, :21-24), correlate(codedData, CODEDFRAMESIZE = 16384)
 * and the three getters (:218-245).  For every consecutive window of `frame`
 * int8 soft symbols: the word with the most agreeing hard bits (first word on a
 * tie), the first position where it reaches that count, and the count
 * (MINCORRELATIONBITS = 46 is the decoder's acceptance, parameters.h:31).
 * word 0 = as sent, word 1 = inverted (PhaseShift::DEG_180, :232). */
typedef struct xrit_sync_hit {
    uint32_t word;
    uint32_t position;
    uint32_t correlation;
    uint32_t reserved;
} xrit_sync_hit;
/* device pointers; hits has n_symbols / frame entries */
int xrit_sync_correlate_device(const int8_t *d_symbols, size_t n_symbols, const uint64_t *words, int nwords,
                               uint32_t frame, xrit_sync_hit *d_hits, int device, void *stream);
/* host buffers (one H2D / D2H round trip) */
int xrit_sync_correlate(const int8_t *symbols, size_t n_symbols, const uint64_t *words, int nwords, uint32_t frame,
                        xrit_sync_hit *hits, int device);

/* Frame alignment and phase fix, the two steps between the correlator and Viterbi
 * (newdecoder.cpp:239-270): for window f the frame that starts at the correlation
 * position, symbols[f*frame + position .. + frame) -- the reference shifts its chunk
 * down and reads `position` more bytes -- with every byte XOR 0xFF when word != 0
 * (PacketFixer::fixPacket(..., DEG_180, false), :232,:265-267; LRIT only: HRIT is
 * differentially coded and skips it, so pass hits with word forced to 0 there).
 * A window whose correlation is below min_correlation (MINCORRELATIONBITS, :239-242)
 * or whose frame would run past n_symbols gives no frame: zeros, valid[f] = 0.
 * frames: (n_symbols / frame) * frame bytes; valid: n_symbols / frame bytes. */
int xrit_sync_fix_frames_device(const int8_t *d_symbols, size_t n_symbols, const xrit_sync_hit *d_hits, uint32_t frame,
                                uint32_t min_correlation, int8_t *d_frames, uint8_t *d_valid, int device, void *stream);
int xrit_sync_fix_frames(const int8_t *symbols, size_t n_symbols, const xrit_sync_hit *hits, uint32_t frame,
                         uint32_t min_correlation, int8_t *frames, uint8_t *valid, int device);

/* ------------------------------------------------------------------------
 * Stream frame synchroniser: the reference decoder's walk over a STREAM of
 * soft symbols (newdecoder.cpp:212-270 with flywheelRecheck = 1), state in
 * device memory.  Exact integer contract: DESIGN.md section 17 and
 * tests/framer_spec.py.  The stream arrives in calls of any length; the
 * handle keeps a cursor c (absolute offset, 0 at start) and the symbols from
 * c on that are not consumed yet (at most 2 * frame - 66).  While
 * c + frame <= symbols received:
 *  - hit = the correlator's answer on stream[c .. c + frame) (as
 *    xrit_sync_correlate gives it for that window);
 *  - hit.correlation < min_correlation: a row with the hit, valid = 0, a zero
 *    frame, start = c; c += frame (:244-247);
 *  - else if c + hit.position + frame runs past the symbols received: stop,
 *    the chunk is walked again in the next call (the reference blocks in
 *    Receive);
 *  - else a row with the hit, valid = 1, start = c + hit.position, the frame
 *    stream[start .. start + frame), every byte XOR 0xFF when hit.word != 0 on
 *    a LRIT handle (HRIT never inverts, :266-270); c = start + frame.
 * The rows do not depend on how the stream is cut into calls.  A call of n
 * symbols emits at most xrit_framer_rows(fr, n) = (n + 2 * frame - 66) / frame
 * rows; the outputs hold that many rows, those from *count on are all-zero
 * with valid = 0 -- what xrit_decoder_decode_device and
 * xrit_demux_process_device treat as absent, so both can be queued behind a
 * push with nf = xrit_framer_rows(fr, n) and no read-back.
 * ------------------------------------------------------------------------ */
typedef struct xrit_framer xrit_framer;
typedef struct xrit_framer_counters {   /* 80 bytes */
    uint64_t symbols;            /* received */
    uint64_t cursor;             /* absolute offset of the next chunk */
    uint64_t rows;               /* emitted, valid or not */
    uint64_t frames;             /* rows with valid = 1 */
    uint64_t dropped_chunks;     /* rows with valid = 0 */
    uint64_t resyncs;            /* frames found at position != 0 */
    uint64_t carry;              /* symbols held for the next call: symbols - cursor */
    uint64_t rewalked_chunks;    /* chunks the joints had to walk again (the walkers' guess of the entry cursor missed) */
    uint64_t adopted_chunks;     /* chunks taken over from a segment walker's record */
    uint64_t calls;
} xrit_framer_counters;
#define XRIT_FRAMER_MAX_SYMBOLS ((size_t)1 << 30)   /* per call */

/* hrit = 0: LRIT words (newdecoder.cpp:21-24), 1: HRIT; frame = 16384, min_correlation = 46 */
int xrit_framer_create(xrit_framer **fr, int hrit, int device);
int xrit_framer_destroy(xrit_framer *fr);
/* frame 65 .. 2^20 symbols, min_correlation 0 .. 64; only before the handle's first push */
int xrit_framer_set_frame(xrit_framer *fr, uint32_t frame, uint32_t min_correlation);
/* chunks per walker segment (0: chosen per call, the power of two up to the square root of the call's chunks); the rows do not depend on it */
int xrit_framer_set_segment(xrit_framer *fr, uint32_t chunks);
/* cursor 0, nothing carried, counters zero; waits for the handle's last call */
int xrit_framer_reset(xrit_framer *fr);
/* rows the outputs of a call of n symbols must hold (0 for a null handle) */
size_t xrit_framer_rows(const xrit_framer *fr, size_t n);
/* device pointers, asynchronous on `stream`, no host synchronisation; cursor and carry are updated on the device.
 * With rows = xrit_framer_rows(fr, n): d_frames rows * frame bytes, d_valid rows bytes, d_hits rows entries (raw, as
 * the correlator found them), d_start rows entries (absolute offsets), d_count one entry: the rows emitted.
 * n <= XRIT_FRAMER_MAX_SYMBOLS; n = 0 is a call like any other (d_symbols may then be null). */
int xrit_framer_push_device(xrit_framer *fr, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                            xrit_sync_hit *d_hits, uint64_t *d_start, uint32_t *d_count, void *stream);
/* host buffers of the same sizes: one upload, one download; returns the rows emitted (>= 0) or an error code (< 0) */
int xrit_framer_push(xrit_framer *fr, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                     uint64_t *start);
/* the counters after the last call; waits for it */
int xrit_framer_stats(xrit_framer *fr, xrit_framer_counters *out);

/* ------------------------------------------------------------------------
 * Decoder: Viterbi27 + NRZ-M (HRIT) + DeRandomizer + 4 x RS(255,223), the
 * per-frame FEC of decoder/src/newdecoder.cpp:272-348 on the frames that
 * xrit_sync_fix_frames[_device] writes (16384 int8 symbols each, valid[nf]).
 * Soft convention: symbol s votes for coded bit 0 with weight s, 0 = erasure
 * (the reference's unsigned 128).  Exact integer contract: DESIGN.md
 * "Frame decoder".
 *  - window (:272-276, :298-300): the last 64 symbols of the most recent
 *    earlier valid frame (across calls; zeros at start and after reset) +
 *    the 16384 frame symbols; a valid = 0 frame neither decodes nor moves it.
 *  - Viterbi (:281): maximum likelihood over the window's 8224 bits, register
 *    taking new bits at its low end, polynomials 0x4F / 0x6D, start metrics
 *    0, ties keep the predecessor ns >> 1, traceback from the first best end
 *    state.  HRIT: NRZ-M over the whole window (:282-284).  Bits 32 .. 8223,
 *    MSB first, are cadu[f][1024] (:297, vitdecData at :305).
 *  - viterbi_errors: window symbols with s * (1 - 2c) < 0, c the re-encoded
 *    decision path (Viterbi27::GetBER, :309).
 *  - derandomise bytes 4 .. 1023 with the CCSDS PN sequence (:304-307), then
 *    RS(255,223) errors-only per interleaved codeword, dual basis
 *    (decode_ccsds, :313-318): block[f][1020] (rsCorrectedData), the VCDU is
 *    block[f][0 .. 892) (:359).  rs_errors = corrected symbols or -1; a -1
 *    codeword passes through.  ok = valid and not all four -1 (:321).
 *  - scid / vcid / counter from block[f][0 .. 5) (:342-348).
 * A valid = 0 frame: zero cadu and block bytes, zero info, rs_errors all -1.
 * ------------------------------------------------------------------------ */
typedef struct xrit_decoder xrit_decoder;   /* Viterbi27 + DeRandomizer + ReedSolomon state (newdecoder.cpp:80,125-131) */
typedef struct xrit_frame_info {
    uint32_t valid;
    uint32_t ok;
    uint32_t viterbi_errors;
    int32_t  rs_errors[4];
    uint32_t scid, vcid, counter;
} xrit_frame_info;

/* hrit = 0: LRIT, 1: HRIT (NRZ-M).  No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_decoder_create(xrit_decoder **d, int hrit, int device);
int xrit_decoder_destroy(xrit_decoder *d);
/* carry back to erasures (lastFrameEnd = 128 everywhere, :141); waits for the handle's last call */
int xrit_decoder_reset(xrit_decoder *d);
/* resident Viterbi windows (waves, each with its own 66 KB of decision scratch) that a call starts at most; a call of
 * more frames walks them windows apart.  0: the default, 8 per compute unit; other values are clamped to 1 .. default.
 * Takes effect from the next call; the outputs do not depend on it. */
int xrit_decoder_set_windows(xrit_decoder *d, uint32_t windows);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation; the carry is updated on
 * the device.  d_cadu: nf * 1024 bytes and d_block: nf * 1020 bytes, both 16-byte aligned; d_info: nf entries.
 * Calls on one handle share its carry and scratch: the caller keeps them in order (one stream, or events). */
int xrit_decoder_decode_device(xrit_decoder *d, const int8_t *d_frames, const uint8_t *d_valid, size_t nf,
                               uint8_t *d_cadu, uint8_t *d_block, xrit_frame_info *d_info, void *stream);
/* host buffers; returns when the outputs are written */
int xrit_decoder_decode(xrit_decoder *d, const int8_t *frames, const uint8_t *valid, size_t nf,
                        uint8_t *cadu, uint8_t *block, xrit_frame_info *info);

/* ------------------------------------------------------------------------
 * Frame lock: the stream frame synchroniser and the decoder as the ONE loop
 * the reference runs (newdecoder.cpp:218-237, 321-338; flywheelRecheck,
 * parameters.h:41, default 4).  Exact integer contract: DESIGN.md section 18
 * and tests/lock_spec.py.  Besides the framer's cursor and carry and the
 * decoder's 64-symbol carry the handle keeps ok (lastFrameOK) and fc
 * (flywheelCount) in device memory, both 0 at start.  The frame is 16384
 * symbols and min_correlation 46.  While c + frame <= symbols received, with
 * the state as it was at the chunk's entry:
 *  1. fc == recheck: ok = 0, fc = 0 (:218-221);
 *  2. ok == 0: the hit over the whole chunk, positions 0 .. frame - 65
 *     (XRIT_LOCK_FULL).  Otherwise the hit over the first frame / 16 symbols,
 *     positions 0 .. frame / 16 - 65: at position 0 it is kept
 *     (XRIT_LOCK_SHORT); anywhere else the whole-chunk hit is taken, ok = 0,
 *     fc = 0 (XRIT_LOCK_MISS, :228-235);
 *  3. fc += 1;
 *  4. hit.correlation < 46: a row with the hit, valid = 0, zeros, start = c;
 *     c += frame; ok is not touched (:244-247);
 *  5. else if c + hit.position + frame runs past the symbols received: stop;
 *     nothing is emitted or consumed and ok, fc keep their values of the
 *     chunk's entry: the chunk is walked again in the next call;
 *  6. else a row with the hit, valid = 1, start = c + hit.position, the frame
 *     (inverted when hit.word != 0 on LRIT), decoded behind the carry exactly
 *     as xrit_decoder does; ok = info.ok (:321-338); c = start + frame.
 * With recheck = 1 the rows are those of xrit_framer followed by xrit_decoder.
 * The rows do not depend on how the stream is cut into calls.  The outputs
 * hold xrit_lock_rows(lk, n) rows; those from *count on are all-zero with
 * valid = 0 (rs_errors -1), so d_hits, d_cadu, d_block and d_info go to
 * xrit_demux_process_device as they are.  mode[r]: XRIT_LOCK_FULL / SHORT /
 * MISS, plus XRIT_LOCK_RECHECK when step 1 fired on the chunk; hits[r] is the
 * hit that was used.
 * ------------------------------------------------------------------------ */
typedef struct xrit_lock xrit_lock;
#define XRIT_LOCK_FULL 0
#define XRIT_LOCK_SHORT 1
#define XRIT_LOCK_MISS 2
#define XRIT_LOCK_RECHECK 4
typedef struct xrit_lock_counters {     /* 136 bytes */
    xrit_framer_counters framer;        /* as xrit_framer_stats gives them; rewalked_chunks counts a chunk once, when it is consumed */
    uint64_t short_kept;                /* chunks taken in mode SHORT */
    uint64_t short_missed;              /* ... in mode MISS */
    uint64_t rechecks;                  /* chunks on which step 1 fired */
    uint64_t sensitive_chunks;          /* whole-chunk hit not at 0, short hit at 0, fc != recheck at entry: the outcome hangs on ok */
    uint64_t rounds;                    /* passes of joints, gather, decoder and commit: calls + the stops for an RS outcome */
    uint64_t frames_ok;                 /* valid rows with info.ok */
    uint64_t frames_bad;                /* valid rows without */
} xrit_lock_counters;

int xrit_lock_create(xrit_lock **lk, int hrit, int device);
int xrit_lock_destroy(xrit_lock *lk);
/* cursor 0, nothing carried, ok = 0, fc = 0, the decoder's carry back to erasures, counters zero; waits for the last call */
int xrit_lock_reset(xrit_lock *lk);
/* flywheelRecheck, 1 .. 255 (default 4; 1: no flywheel); only before the handle's first push -- xrit_lock_reset does not
 * reopen it: a handle keeps its recheck for life once it has pushed */
int xrit_lock_set_flywheel(xrit_lock *lk, uint32_t recheck);
/* as xrit_framer_set_segment and xrit_decoder_set_windows; the outputs do not depend on them */
int xrit_lock_set_segment(xrit_lock *lk, uint32_t chunks);
int xrit_lock_set_windows(xrit_lock *lk, uint32_t windows);
/* rows the outputs of a call of n symbols must hold: xrit_framer_rows at frame 16384 (0 for a null handle) */
size_t xrit_lock_rows(const xrit_lock *lk, size_t n);
/* device pointers; the work is queued on `stream`, and the call SYNCHRONISES that stream once per round to read back one
 * small record (rows so far, stopped or done): a round ends where the walk needs the RS outcome of a row the round
 * itself emitted, so a call is 1 + (such stops) rounds, one on a stream in lock.  That read-back is the price of the
 * coupling; no value goes from the host to the device between rounds.  With rows = xrit_lock_rows(lk, n): d_frames
 * rows * 16384 bytes, d_valid rows, d_hits rows, d_start rows, d_mode rows bytes, d_cadu rows * 1024 (16-byte aligned),
 * d_block rows * 1020, d_info rows, d_count one entry.  n <= XRIT_FRAMER_MAX_SYMBOLS; n = 0 is a call like any other. */
int xrit_lock_push_device(xrit_lock *lk, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                          xrit_sync_hit *d_hits, uint64_t *d_start, uint8_t *d_mode, uint8_t *d_cadu, uint8_t *d_block,
                          xrit_frame_info *d_info, uint32_t *d_count, void *stream);
/* host buffers of the same sizes; returns the rows emitted (>= 0) or an error code (< 0) */
int xrit_lock_push(xrit_lock *lk, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                   uint64_t *start, uint8_t *mode, uint8_t *cadu, uint8_t *block, xrit_frame_info *info);
/* the counters after the last call; waits for it */
int xrit_lock_stats(xrit_lock *lk, xrit_lock_counters *out);

/* ------------------------------------------------------------------------
 * Channel demultiplexer and packet accounting: the last stage of the
 * reference decoder's data path (decoder/src/newdecoder.cpp:309-395), on the
 * decoder's outputs.  Exact integer contract: DESIGN.md "Channel demux".
 *  - per call, in frame order: the correlator's hit as it returned it (the
 *    phase of a LRIT frame), the frame's cadu (syncWord = cadu[0 .. 4), :302),
 *    its block and its xrit_frame_info.  A valid = 0 frame does not exist
 *    for this stage (:244-247).
 *  - a good frame (ok) adds its VCDU block[0 .. 892) to channel vcid
 *    (ChannelWriter::writeChannel, :356-360; VCID 63 is not filtered) and
 *    runs the lost-packet test of :363-371 on 24-bit counters with the
 *    reference's C types: a counter wrap adds -2^24, a repeated counter -1.
 *  - every valid frame leaves one Statistics_st (Statistics.h:14-36), the
 *    record StatisticsDispatcher sends (:373-395); xrit_frame_stats is its
 *    compact form, xrit_demux_expand writes the 4167-byte wire form.
 * The counters carry across calls on one handle until reset.
 * ------------------------------------------------------------------------ */
typedef struct xrit_demux xrit_demux;
/* the counters of newdecoder.cpp:44-53 after a call (the 256-wide arrays as Statistics_st holds them; entries
 * 64 .. 255 stay at their start values, vcid has 6 bits) */
typedef struct xrit_decoder_stats {
    uint64_t total_packets;          /* frameCount: valid frames */
    uint64_t dropped_packets;        /* droppedPackets: valid frames with all four RS codewords -1 */
    uint64_t lost_packets;           /* lostPackets (uint64, wraps) */
    uint64_t sum_viterbi_errors;     /* the averageVitCorrections accumulator */
    uint64_t sum_rs_corrections;     /* the averageRSCorrections accumulator */
    int64_t  received[256];          /* receivedPacketsPerFrame: -1 until a channel's first good frame */
    int64_t  lost[256];              /* lostPacketsPerFrame */
    int64_t  last_counter[256];      /* lastPacketCount: -1 until a channel's first good frame */
    uint32_t start_time;             /* Statistics_st::startTime: the handle's creation, Unix seconds */
    uint32_t reserved;
} xrit_decoder_stats;
/* Statistics_st after one frame, without the arrays: every scalar, plus the frame's VCID entries of the two arrays.
 * A frame that is not good has scid = vcid = packet_number = signal_quality = phase_correction = 0, frame_lock = 0
 * and received_vc = lost_vc = 0 (its record changes no array entry); a valid = 0 frame has an all-zero record. */
typedef struct xrit_frame_stats {
    uint64_t packet_number;          /* the 24-bit counter */
    uint64_t lost_packets;
    uint64_t dropped_packets;
    uint64_t total_packets;
    int64_t  received_vc;            /* receivedPacketsPerChannel[vcid] after the frame */
    int64_t  lost_vc;                /* lostPacketsPerChannel[vcid] after the frame */
    int32_t  rs_errors[4];
    uint16_t vit_errors;             /* (uint16) viterbi_errors */
    uint16_t frame_bits;             /* 8192 */
    uint16_t average_vit_corrections;
    uint8_t  scid, vcid;
    uint8_t  signal_quality;         /* uint8(max(0, 100 - 10 * (100 * viterbi_errors / 8256))) in float32 */
    uint8_t  sync_correlation;       /* (uint8) hit.correlation */
    uint8_t  phase_correction;       /* hit.word ? 180 : 0 */
    uint8_t  average_rs_corrections;
    uint8_t  sync_word[4];
    uint8_t  frame_lock;
    uint8_t  valid;
    uint8_t  reserved[6];
} xrit_frame_stats;                  /* 88 bytes */
#define XRIT_STATISTICS_WIRE_BYTES 4167   /* sizeof(Statistics_st), packed */

int xrit_demux_create(xrit_demux **dm, int device);
int xrit_demux_destroy(xrit_demux *dm);
/* the start state of newdecoder.cpp:133-137 (startTime is kept); waits for the handle's last call */
int xrit_demux_reset(xrit_demux *dm);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation; it may be queued directly
 * behind xrit_decoder_decode_device.  nf <= 2^24.  d_hits, d_info, d_records: nf entries; d_cadu: nf * 1024 bytes;
 * d_block: nf * 1020 bytes; d_vcdu: room for nf * 892 bytes (the good frames' VCDUs grouped by VCID in ascending
 * order, frame order within a VCID; rows d_offsets[v] .. d_offsets[v + 1] are channel v's); d_offsets: 65 entries.
 * d_cadu, d_block and d_vcdu 4-byte aligned.  Calls on one handle share its state and scratch: keep them in order. */
int xrit_demux_process_device(xrit_demux *dm, const xrit_sync_hit *d_hits, const uint8_t *d_cadu, const uint8_t *d_block,
                              const xrit_frame_info *d_info, size_t nf, uint8_t *d_vcdu, uint32_t *d_offsets,
                              xrit_frame_stats *d_records, void *stream);
/* host buffers (one upload, one download); returns when the outputs are written */
int xrit_demux_process(xrit_demux *dm, const xrit_sync_hit *hits, const uint8_t *cadu, const uint8_t *block,
                       const xrit_frame_info *info, size_t nf, uint8_t *vcdu, uint32_t *offsets, xrit_frame_stats *records);
/* the full counters after the handle's last call (waits for it) */
int xrit_demux_stats(xrit_demux *dm, xrit_decoder_stats *out);
/* plain host code: from the counters before a call and that call's records, one XRIT_STATISTICS_WIRE_BYTES record per
 * valid frame into out (packed, little-endian, Statistics.h's field order: what StatisticsDispatcher sends).
 * Returns the number of records written, or a negative XRIT_E_* code. */
int xrit_demux_expand(const xrit_decoder_stats *start, const xrit_frame_stats *records, size_t nf, uint8_t *out);

/* ------------------------------------------------------------------------
 * Packet assembler: CCSDS space packets (the LRIT/HRIT CP_PDUs) out of the
 * demultiplexer's VCDU rows, with CRC.  The reference decoder ends at the VCDU,
 * so there is no reference line to cite: the layout is taken from the CCSDS
 * AOS space data link recommendation (CCSDS 732.0-B: the M_PDU, its first
 * header pointer, 2047 = no header, 2046 = idle data), the space packet
 * recommendation (CCSDS 133.0-B: the 6-byte primary header, APID 2047 = idle
 * packet) and the LRIT/HRIT global specification (CGMS 03: the CP_PDU's
 * CRC-16 over its data field).  Exact integer contract: DESIGN.md "Packet
 * assembler"; tests/packet_spec.py is the serial statement of it.
 *  - input: the demux's vcdu rows (892 bytes, grouped by VCID) and offsets[65].
 *    Channel 63 (fill VCDUs) is ignored.  In a row r: counter = r[2..5) big
 *    endian, fhp = (r[6] & 7) << 8 | r[7], packet zone = r[8..892).
 *  - per channel, carried across calls until reset: the last row's counter and
 *    the bytes of a packet that has begun and not ended.  A break in the
 *    counters drops that partial packet; the first header pointer is
 *    authoritative (what it contradicts is dropped, never re-interpreted).
 *  - a finished packet of APID 2047 is counted and not emitted; every other one
 *    is emitted whole (header included) with one xrit_packet descriptor.
 *    crc_ok = 1 iff length >= 8 and the big-endian 16 bits in its last two
 *    bytes are CRC-16/CCITT-FALSE (0x1021, initial value 0xFFFF, MSB first) of
 *    packet[6 .. length - 2).  A packet that fails is still emitted.
 *  - output order: VCID ascending, stream order within a VCID.
 * ------------------------------------------------------------------------ */
typedef struct xrit_packets xrit_packets;
typedef struct xrit_packet {
    uint64_t offset;                 /* of the packet's first byte in the call's byte buffer */
    uint32_t length;                 /* 7 + the header's length field: primary header included (7 .. 65542) */
    uint32_t first_counter;          /* VCDU counter of the row the packet began in */
    uint16_t apid;                   /* (h[0] & 7) << 8 | h[1] */
    uint16_t seq_count;              /* (h[2] & 0x3F) << 8 | h[3] */
    uint16_t crc_computed;           /* 0 when length < 8 */
    uint16_t crc_carried;            /* the last two bytes, big endian; 0 when length < 8 */
    uint8_t  vcid;
    uint8_t  seq_flags;              /* h[2] >> 6 */
    uint8_t  crc_ok;
    uint8_t  header_bits;            /* h[0] >> 3: version, type, secondary header flag, not interpreted */
    uint8_t  reserved[4];
} xrit_packet;                       /* 32 bytes */
typedef struct xrit_packets_summary {
    uint64_t packets, bytes;         /* emitted by this call: the true counts, whatever the capacities */
    uint64_t total_packets, crc_failures, fill_packets, discarded, bad_fhp, rows;   /* the handle's counters after it */
    uint32_t overflow;               /* 0; 1: max_packets or max_bytes too small; 2: d_offsets[64] > max_rows */
    uint32_t reserved;
} xrit_packets_summary;              /* 72 bytes */
typedef struct xrit_packets_counters {
    uint64_t packets, crc_failures, fill_packets, discarded, bad_fhp, rows;         /* all channels */
    uint64_t vc_packets[64], vc_crc_failures[64], vc_fill_packets[64], vc_discarded[64], vc_bad_fhp[64], vc_rows[64];
    int64_t  last_counter[64];       /* -1 until a channel's first row */
    uint32_t pending_bytes[64];      /* bytes held of a packet that has begun and not ended (0 .. 65541) */
    uint32_t pending_first_counter[64];
} xrit_packets_counters;             /* 4144 bytes */
/* the bytes of a call never exceed this */
#define XRIT_PACKETS_MAX_BYTES(rows) ((size_t)884 * (rows) + (size_t)65541 * 64)

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_packets_create(xrit_packets **pa, int device);
int xrit_packets_destroy(xrit_packets *pa);
/* every channel back to its start (no last counter, nothing pending, counters zero); waits for the handle's last call */
int xrit_packets_reset(xrit_packets *pa);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_demux_process_device, which hands it its row count in d_offsets[64] on the device.  max_rows (<= 2^24)
 * is the host's bound on that count (the demux call's nf): launches and scratch are sized from it; a larger
 * d_offsets[64] raises overflow = 2 in the summary (packets = bytes = 0, the counters the handle's) and all 65
 * entries of d_pkt_offsets are written as zeros, so that a files call queued behind sees no packets; nothing else is
 * written, the state unchanged.
 * d_bytes: max_bytes; d_packets: max_packets descriptors, 8-byte aligned; d_pkt_offsets: 65 entries, the exclusive
 * prefix of the per-channel packet counts; d_summary: 8-byte aligned.  Capacity: descriptor k is written iff
 * k < max_packets, a packet's bytes iff offset + length <= max_bytes; the summary carries the true counts and
 * overflow = 1, and the handle's state advances as if everything had fitted.
 * Calls on one handle share its state and scratch: keep them in order. */
int xrit_packets_process_device(xrit_packets *pa, const uint8_t *d_vcdu, const uint32_t *d_offsets, size_t max_rows,
                                uint8_t *d_bytes, size_t max_bytes, xrit_packet *d_packets, size_t max_packets,
                                uint32_t *d_pkt_offsets, xrit_packets_summary *d_summary, void *stream);
/* host buffers (one upload, one download); the rows are offsets[64].  XRIT_E_CAPACITY when a capacity was too small:
 * the prefix that fits is written, summary and pkt_offsets are the true ones, the state has advanced. */
int xrit_packets_process(xrit_packets *pa, const uint8_t *vcdu, const uint32_t *offsets, uint8_t *bytes, size_t max_bytes,
                         xrit_packet *packets, size_t max_packets, uint32_t *pkt_offsets, xrit_packets_summary *summary);
/* the full counters after the handle's last call (waits for it) */
int xrit_packets_stats(xrit_packets *pa, xrit_packets_counters *out);

/* ------------------------------------------------------------------------
 * File assembler and Rice decoder: LRIT/HRIT files out of the packet
 * assembler's space packets, and the Rice-coded scan lines inside GOES image
 * files.  The reference decoder ends at the VCDU, so there is no reference line
 * to cite: the layouts are taken from the space packet recommendation (CCSDS
 * 133.0-B: sequence flags 1 first, 0 continuation, 2 last, 3 unsegmented; the
 * 14-bit sequence count), the LRIT/HRIT global specification (CGMS 03: the
 * transport file's 10-byte header -- file counter, length in bits --, the
 * primary header record, the image structure record, type 1), the GOES
 * mission specific Rice compression record (type 131) and the lossless data
 * compression recommendation (CCSDS 121.0-B: the adaptive entropy coder and
 * the unit-delay predictor).  No libaec and no recorded downlink was at hand:
 * DESIGN.md sections 15 and 16 list what is unverified.  Exact integer
 * contracts there; tests/file_spec.py and tests/rice_spec.py are the serial
 * statements.
 *
 * Files.  Input: one packets call's bytes, descriptors and pkt_offsets[65].
 *  - key = (vcid, apid); per key, carried across calls until reset: whether a
 *    file is open, the next sequence count, the file's serial on its key, its
 *    bytes and pieces so far, the transport header and the parsed header fields.
 *    File bytes are not kept: a call emits the pieces it saw.
 *  - a packet is bad iff crc_ok == 0, length < 8 or it lies outside the input
 *    bytes; a bad packet, a break in the sequence counts or a new first packet
 *    aborts the open file (its record carries ABORTED; nothing emitted is taken
 *    back).  Pieces outside a file are counted (orphans) and not emitted.
 *  - outputs ordered by (vcid, apid, stream order): the pieces' payloads back to
 *    back, one xrit_file_piece each, one xrit_file_record per file touched.
 * ------------------------------------------------------------------------ */
#define XRIT_E_ARG XRIT_E_INVALID   /* the argument-error code under the name the file / Rice stages' documents use */
typedef struct xrit_files xrit_files;
typedef struct xrit_file_piece {
    uint64_t offset;                 /* of the payload's first byte in the call's byte buffer */
    uint32_t length;                 /* payload bytes (0 .. 65528) */
    uint32_t index_in_file;          /* 0 for the piece that began the file */
    uint32_t file;                   /* index into the call's records */
    uint16_t seq_count, apid;
    uint8_t  vcid, seq_flags;
    uint8_t  reserved[6];
} xrit_file_piece;                   /* 32 bytes; begins like xrit_packet: either serves as a Rice line descriptor */
#define XRIT_FILE_BEGINS       1     /* the file's first piece is in this call */
#define XRIT_FILE_ENDS         2     /* ... its last */
#define XRIT_FILE_ABORTED      4     /* the host discards the file */
#define XRIT_FILE_LENGTH_MATCH 8     /* on ENDS: 8 * (file_offset + length) == declared_bits */
typedef struct xrit_file_record {
    uint64_t offset, length;         /* the file's bytes of this call: contiguous in the call's byte buffer */
    uint64_t file_offset;            /* bytes of the file emitted by earlier calls */
    uint64_t declared_bits;          /* transport header: BE64(u[2..10)); reported, never used to cut */
    uint64_t data_bits;              /* primary header */
    uint32_t header_length;          /* primary header: total header length */
    uint32_t first_piece, n_pieces;  /* this call's pieces of the file */
    uint32_t key_serial;             /* files begun on this key before this one */
    uint16_t file_counter;           /* transport header: BE16(u[0..2)) */
    uint16_t apid;
    uint16_t columns, lines;         /* image structure record (type 1, length 9) */
    uint16_t rice_flags;             /* Rice record (type 131, length 7) */
    uint8_t  vcid, flags;
    uint8_t  file_type;              /* primary header */
    uint8_t  header_state;           /* 0: no primary header in the first piece; 1: headers incomplete or malformed; 2: walked to their end */
    uint8_t  bits_per_pixel, compression;
    uint8_t  pixels_per_block, lines_per_packet;
    uint8_t  reserved[6];
} xrit_file_record;                  /* 80 bytes */
typedef struct xrit_files_counters {
    uint64_t files_begun, files_completed, files_aborted, bad_packets, seq_gaps, short_first, orphans;
    uint64_t total_pieces, total_bytes;
    uint64_t open_files;             /* keys with a file open */
} xrit_files_counters;               /* 80 bytes */
typedef struct xrit_files_summary {
    uint64_t pieces, bytes, files;   /* of this call: the true counts, whatever the capacities */
    uint64_t files_begun, files_completed, files_aborted, bad_packets, seq_gaps, short_first, orphans;   /* the handle's */
    uint64_t total_pieces, total_bytes;                                                                  /* counters after it */
    uint32_t overflow;               /* 0; 1: a capacity too small; 2: d_pkt_offsets[64] > max_packets_in */
    uint32_t reserved;
} xrit_files_summary;                /* 104 bytes */
/* what one key carries (xrit_files_key) */
typedef struct xrit_file_key {
    uint64_t file_bytes, declared_bits, data_bits;
    uint32_t header_length, n_pieces, key_serial;
    uint16_t next_seq, file_counter, columns, lines, rice_flags;
    uint8_t  open, file_type, header_state, bits_per_pixel, compression, pixels_per_block, lines_per_packet;
    uint8_t  reserved[3];
} xrit_file_key;                     /* 56 bytes */
#define XRIT_FILES_MAX_PACKETS ((size_t)1 << 24)            /* packets per call */
/* a call on n packets of b bytes emits at most n pieces, b bytes and 2 n records (in fact n + one per key) */
#define XRIT_FILES_MAX_PIECES(n) ((size_t)(n))
#define XRIT_FILES_MAX_BYTES(b)  ((size_t)(b))
#define XRIT_FILES_MAX_FILES(n)  ((size_t)2 * (n))

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_files_create(xrit_files **fa, int device);
int xrit_files_destroy(xrit_files *fa);
/* every key back to its start, counters zero; waits for the handle's last call */
int xrit_files_reset(xrit_files *fa);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_packets_process_device, which hands it its packet count in d_pkt_offsets[64] on the device.
 * max_packets_in (<= XRIT_FILES_MAX_PACKETS) is the host's bound on that count (the descriptors the packets call could
 * write: its max_packets), in_bytes the size of d_in_bytes (its max_bytes): a larger d_pkt_offsets[64] raises
 * overflow = 2 and nothing else is written, the state unchanged; a packet that lies outside in_bytes is a bad packet.
 * d_pieces, d_files, d_summary 8-byte aligned.  Capacity: piece k is written iff k < max_pieces, its bytes iff offset +
 * length <= max_bytes, record k iff k < max_files; the summary carries the true counts and overflow = 1, and the
 * handle's state advances as if everything had fitted.  Calls on one handle share its state and scratch: keep them in
 * order. */
int xrit_files_process_device(xrit_files *fa, const uint8_t *d_in_bytes, size_t in_bytes, const xrit_packet *d_packets,
                              const uint32_t *d_pkt_offsets, size_t max_packets_in, uint8_t *d_bytes, size_t max_bytes,
                              xrit_file_piece *d_pieces, size_t max_pieces, xrit_file_record *d_files, size_t max_files,
                              xrit_files_summary *d_summary, void *stream);
/* host buffers (one upload, one download); the packets are pkt_offsets[64].  XRIT_E_CAPACITY when a capacity was too
 * small: the prefix that fits is written, the summary is the true one, the state has advanced. */
int xrit_files_process(xrit_files *fa, const uint8_t *in_bytes, size_t n_in_bytes, const xrit_packet *packets,
                       const uint32_t *pkt_offsets, uint8_t *bytes, size_t max_bytes, xrit_file_piece *pieces,
                       size_t max_pieces, xrit_file_record *files, size_t max_files, xrit_files_summary *summary);
/* the counters after the handle's last call (waits for it) */
int xrit_files_stats(xrit_files *fa, xrit_files_counters *out);
/* what key (vcid < 64, apid < 2048) carries after the handle's last call (waits for it) */
int xrit_files_key(xrit_files *fa, unsigned vcid, unsigned apid, xrit_file_key *out);

/* Rice.  A batch of coded lines, each decoded on its own: n_lines descriptors `stride` bytes apart (stride >= 16, a
 * multiple of 8), each beginning {uint64 offset; uint32 length} into d_bytes -- xrit_packet and xrit_file_piece both
 * fit.  bits_per_sample 1 .. 16, block 8 / 16 / 32 / 64, samples 1 .. 65535 per line: anything else XRIT_E_ARG.
 * d_out: n_lines * samples of uint8 (bits_per_sample <= 8) or little-endian uint16; d_status[n_lines]: 0, 1 (a fault:
 * the blocks decoded in front of it are kept, the rest 0) or 2 (the descriptor points outside the n_bytes of d_bytes
 * or is longer than 2^20 bytes: nothing read, all 0).  Stateless: no handle, no scratch.  Asynchronous on `stream`, no
 * host synchronisation. */
int xrit_rice_decode_device(const uint8_t *d_bytes, size_t n_bytes, const void *d_desc, size_t stride, size_t n_lines,
                            int bits_per_sample, int block, int samples, void *d_out, uint8_t *d_status, int device,
                            void *stream);
/* Which kernel the decode calls launch, process wide: the default is the wave form (DESIGN.md section 16 has
 * what was measured); the other stays selectable so that tests and the benchmark hold both to the specification.  LANE: one lane per
 * line; WAVE: one wave per line.  Anything else: XRIT_E_ARG. */
#define XRIT_RICE_FORM_DEFAULT 0
#define XRIT_RICE_FORM_LANE    1
#define XRIT_RICE_FORM_WAVE    2
int xrit_rice_form(int form);
/* host buffers (one upload, one download; staged through grow-only device buffers that the calling thread keeps) */
int xrit_rice_decode(const uint8_t *bytes, size_t n_bytes, const void *desc, size_t stride, size_t n_lines,
                     int bits_per_sample, int block, int samples, void *out, uint8_t *status, int device);

/* ------------------------------------------------------------------------
 * Image lines: every Rice-coded line of every image file in one files call,
 * decoded in one pass (tests/image_spec.py is the serial
 * statement).  Input: a files call's bytes, pieces, records and summary; the
 * true counts are read from the summary on the device.
 *  - key = (vcid, apid); per key, carried across calls until reset: whether a
 *    rice-coded image is open, its key_serial, its lines and faults so far.
 *  - a record with BEGINS is rice iff the link rule of section 16 holds
 *    (header_state 2, file_type 0, compression 1, bits_per_pixel 1 .. 16,
 *    columns >= 1, pixels_per_block 8 / 16 / 32 / 64, header_length == the first
 *    piece's length); its lines are its pieces behind the first.  A record
 *    without BEGINS is rice iff the key's state is open with the record's
 *    key_serial (and the record's parameters are in those ranges); its lines are
 *    all its pieces.  A line is one piece: row = index_in_file - 1, decoded as
 *    xrit_rice_decode does with (bits_per_pixel, pixels_per_block, columns) of
 *    the record, status 0 / 1 / 2 as there.  The record's `lines` field is never
 *    used to cut; lines behind a fault are still decoded.
 *  - after the call the key's state is that of its last record in the call: open
 *    iff it is rice and carries neither ENDS nor ABORTED.
 *  - outputs in piece order: the samples (uint8 for bits <= 8, else little-endian
 *    uint16) back to back, every line padded with zeros to a multiple of 4
 *    bytes; one xrit_image_line per line; one xrit_image_file per files record
 *    (same index; all zero where the record is not rice).
 * ------------------------------------------------------------------------ */
typedef struct xrit_images xrit_images;
typedef struct xrit_image_line {
    uint64_t offset;                 /* of the line's first sample in the call's image bytes (a multiple of 4) */
    uint32_t length;                 /* samples * (1 or 2) bytes, unpadded */
    uint32_t row;                    /* in its image: index_in_file - 1 */
    uint32_t file;                   /* index into the call's records */
    uint32_t piece;                  /* index into the call's pieces */
    uint16_t samples;                /* the record's columns */
    uint8_t  bits;                   /* the record's bits_per_pixel */
    uint8_t  status;                 /* 0; 1: a fault, the blocks in front of it kept, the rest 0; 2: the piece lies outside the bytes, all 0 */
    uint8_t  reserved[4];
} xrit_image_line;                   /* 32 bytes; begins {offset, length} like xrit_packet and xrit_file_piece */
typedef struct xrit_image_file {
    uint64_t offset, length;         /* the record's lines of this call in the image bytes: contiguous, padded lines */
    uint32_t first_line, n_lines;    /* ... and among the call's xrit_image_line */
    uint32_t first_row;              /* the row of the first of them (with no line: the image's lines before this call) */
    uint32_t faults;                 /* lines of this call with status != 0 */
    uint32_t lines_total, faults_total;  /* of the image after this call */
    uint16_t columns;
    uint8_t  bits;
    uint8_t  rice;                   /* 1: the record is a rice-coded image's; 0: every field is 0 */
    uint8_t  reserved[4];
} xrit_image_file;                   /* 48 bytes */
typedef struct xrit_images_counters {
    uint64_t images_begun, images_completed, images_aborted, total_lines, total_faults, total_bytes;
} xrit_images_counters;              /* 48 bytes */
typedef struct xrit_images_summary {
    uint64_t lines, bytes, images;   /* of this call: lines, padded bytes, rice records -- the true counts, whatever the capacities */
    uint64_t images_begun, images_completed, images_aborted, total_lines, total_faults, total_bytes;   /* the handle's counters after it */
    uint32_t overflow;               /* 0; 1: a capacity too small; 2: the files summary has overflow != 0 or counts beyond the host's bounds */
    uint32_t reserved;
} xrit_images_summary;               /* 80 bytes */
/* what one key carries (xrit_images_key) */
typedef struct xrit_image_key {
    uint32_t key_serial, lines, faults;
    uint8_t  open;
    uint8_t  reserved[3];
} xrit_image_key;                    /* 16 bytes */
#define XRIT_IMAGES_MAX_PIECES ((size_t)1 << 24)            /* bounds on a call's pieces ... */
#define XRIT_IMAGES_MAX_FILES  ((size_t)1 << 25)            /* ... and records */
/* a call on p pieces emits at most p lines; a line is at most 65535 samples of 2 bytes, padded: 131072 bytes */
#define XRIT_IMAGES_MAX_LINES(p) ((size_t)(p))
#define XRIT_IMAGES_MAX_BYTES(p) ((size_t)131072 * (p))

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_images_create(xrit_images **im, int device);
int xrit_images_destroy(xrit_images *im);
/* every key closed, counters zero; waits for the handle's last call */
int xrit_images_reset(xrit_images *im);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_files_process_device, whose d_bytes (n_bytes: its max_bytes), d_pieces (max_pieces_in: its max_pieces),
 * d_files (max_files_in: its max_files) and d_summary it takes.  If that summary has overflow != 0 or counts beyond
 * these bounds, only d_summary is written, with overflow = 2, and the state is unchanged.  d_image_files has
 * max_files_in entries.  d_out, d_pieces, d_files, d_lines, d_image_files and both summaries 8-byte aligned.  Capacity:
 * line k is written iff k < max_lines, its samples iff offset + padded length <= max_bytes; the summary carries the
 * true counts and overflow = 1, and the handle's state advances as if everything had fitted.  Calls on one handle
 * share its state and scratch: keep them in order. */
int xrit_images_process_device(xrit_images *im, const uint8_t *d_bytes, size_t n_bytes, const xrit_file_piece *d_pieces,
                               size_t max_pieces_in, const xrit_file_record *d_files, size_t max_files_in,
                               const xrit_files_summary *d_files_summary, uint8_t *d_out, size_t max_bytes,
                               xrit_image_line *d_lines, size_t max_lines, xrit_image_file *d_image_files,
                               xrit_images_summary *d_summary, void *stream);
/* host buffers (one upload, one download): what xrit_files_process returned; n_pieces_in and n_files_in are the lengths
 * of the arrays handed over (the device's bounds).  image_files has n_files_in entries.  XRIT_E_CAPACITY when a
 * capacity was too small: the prefix that fits is written, the summary is the true one, the state has advanced.
 * XRIT_E_ARG with summary->overflow = 2 when the call was refused (nothing else written). */
int xrit_images_process(xrit_images *im, const uint8_t *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t n_pieces_in,
                        const xrit_file_record *files, size_t n_files_in, const xrit_files_summary *files_summary,
                        uint8_t *out, size_t max_bytes, xrit_image_line *lines, size_t max_lines, xrit_image_file *image_files,
                        xrit_images_summary *summary);
/* the counters after the handle's last call (waits for it) */
int xrit_images_stats(xrit_images *im, xrit_images_counters *out);
/* what key (vcid < 64, apid < 2048) carries after the handle's last call (waits for it) */
int xrit_images_key(xrit_images *im, unsigned vcid, unsigned apid, xrit_image_key *out);

/* ------------------------------------------------------------------------
 * Image canvases: the decoded lines of one files call and the images call on it,
 * placed into full images in device memory (DESIGN.md section 20;
 * tests/canvas_spec.py is the serial statement).  GOES sends an image as several
 * segment files; each carries a segment identification record (mission
 * specific, type 128, length 17; seven big-endian 16-bit fields: image_id,
 * segment, start_column, start_line, max_segment, max_column, max_row) that says
 * where its rows belong.  UNVERIFIED, our reading, no recorded downlink and no
 * other implementation at hand: that layout; that the segments of one image
 * share vcid and image_id, possibly on different apids; that start_line and
 * start_column count from 0.
 *  - the handle owns `slots` canvases of slot_bytes each, all zero while free.
 *  - the records are taken in record order.  A record with BEGINS whose
 *    xrit_image_file.rice is 1: the headers in its first piece are walked (as the
 *    file stage walks them) for the first record 128 of length 17 and the first
 *    annotation record (type 4; its first 64 bytes, zero padded, are the name).
 *    Without record 128 the file is an image of one segment: image_id 0xFFFFFFFF
 *    (never joins), segment = max_segment = 1, start (0, 0), max_column = columns,
 *    max_row = lines of the image structure record.  Then, in this order:
 *      BAD_SEGMENT   max_segment 0 or > 64; segment 0 or > max_segment; max_column,
 *                    max_row or the record's lines 0; start_column + columns >
 *                    max_column; start_line + lines > max_row
 *      TOO_LARGE     pitch * max_row > slot_bytes; pitch = (max_column * width + 3)
 *                    & ~3, width 1 for bits <= 8, else 2
 *      a slot in use with the same (vcid, image_id, max_column, max_row,
 *      max_segment, bits), image_id != 0xFFFFFFFF -- the apid is not part of it:
 *      DUPLICATE     the segment's bit is set in begun_mask
 *      OVERLAP       its rectangle meets that of a segment begun there
 *                    otherwise it joins
 *      no such slot: the free slot of lowest index is born;
 *      NO_SLOT       none is free
 *    On success the key (vcid, apid) carries the placement (xrit_canvas_key_state); a
 *    BEGINS record that is not rice, or that was refused, leaves it without one.
 *  - a rice record without BEGINS is placed iff the key's state has `placed` with
 *    the record's key_serial and the slot is in use with the same generation;
 *    otherwise NO_PLACEMENT.
 *  - every xrit_image_line of a placed record, whatever its status, is copied as
 *    the image stage wrote it: `length` bytes to slot base + (start_line + row) *
 *    pitch + start_column * width.  A line with row >= the segment's declared
 *    lines (or one that the inputs do not hold whole) is counted clipped.  No two
 *    lines ever write one pixel, so the canvas is deterministic without atomics.
 *  - ENDS sets the segment's bit in done_mask, ABORTED in aborted_mask (its rows
 *    stay; the segment is never accepted again); complete iff done_mask covers
 *    1 .. max_segment.
 * ------------------------------------------------------------------------ */
typedef struct xrit_canvas xrit_canvas;
#define XRIT_CANVAS_NOT_RICE     0   /* the image stage said so: every field of the xrit_canvas_file is 0 */
#define XRIT_CANVAS_PLACED       1
#define XRIT_CANVAS_BAD_SEGMENT  2
#define XRIT_CANVAS_TOO_LARGE    3
#define XRIT_CANVAS_DUPLICATE    4
#define XRIT_CANVAS_OVERLAP      5
#define XRIT_CANVAS_NO_SLOT      6
#define XRIT_CANVAS_NO_PLACEMENT 7
#define XRIT_CANVAS_NO_ID        0xFFFFFFFFu
#define XRIT_CANVAS_MAX_SLOTS    64
#define XRIT_CANVAS_MAX_SEGMENTS 64
typedef struct xrit_canvas_file {
    int32_t  slot;                   /* -1: none (refused); 0 with reason NOT_RICE */
    uint32_t reason;                 /* XRIT_CANVAS_* */
    uint32_t segment;                /* of a placed record, 1 .. max_segment */
    uint32_t start_line, start_column;
    uint32_t lines_placed, lines_clipped;    /* of this call */
    uint32_t faults;                 /* placed lines of this call with status != 0 */
} xrit_canvas_file;                  /* 32 bytes */
typedef struct xrit_canvas_slot {
    uint64_t begun_mask, done_mask, aborted_mask;    /* bit segment - 1 */
    uint32_t image_id;
    uint32_t max_column, max_row, max_segment;
    uint32_t pitch;                  /* bytes per canvas row */
    uint32_t lines_placed, faults;   /* over the slot's segments */
    uint32_t generation;             /* releases of this slot */
    uint32_t born_call, touched_call;    /* the handle's call counter: 1 for its first call */
    uint8_t  in_use, complete, vcid, bits;
    uint8_t  reserved[4];
    uint8_t  name[64];               /* the annotation text, zero padded */
} xrit_canvas_slot;                  /* 136 bytes */
typedef struct xrit_canvas_segment {
    uint32_t start_line, start_column, lines, columns;
    uint32_t placed, faults;         /* lines placed so far; those with status != 0 */
    uint32_t key_serial;             /* of its file on (slot's vcid, apid) */
    uint16_t apid;
    uint8_t  begun;
    uint8_t  reserved;
} xrit_canvas_segment;               /* 32 bytes */
/* what one key carries (xrit_canvas_key reads it) */
typedef struct xrit_canvas_key_state {
    uint32_t key_serial, slot, generation, segment, start_line, start_column;
    uint32_t lines;                  /* the segment's declared lines */
    uint8_t  placed;
    uint8_t  reserved[3];
} xrit_canvas_key_state;                   /* 32 bytes */
typedef struct xrit_canvas_counters {
    uint64_t calls;                  /* calls that were not refused */
    uint64_t canvases_begun, canvases_completed, segments_begun, segments_done, segments_aborted;
    uint64_t lines_placed, lines_clipped, faults;
    uint64_t bad_segment, too_large, duplicate, overlap, no_slot, no_placement;
} xrit_canvas_counters;              /* 120 bytes */
typedef struct xrit_canvas_summary {
    uint64_t placed;                 /* of this call: records placed, */
    uint64_t call_lines_placed, call_lines_clipped, call_faults;     /* their lines, */
    uint64_t completed;              /* canvases that became complete */
    uint64_t calls;                  /* the handle's counters after it */
    uint64_t canvases_begun, canvases_completed, segments_begun, segments_done, segments_aborted;
    uint64_t lines_placed, lines_clipped, faults;
    uint64_t bad_segment, too_large, duplicate, overlap, no_slot, no_placement;
    uint32_t overflow;               /* 0; 2: a summary handed over has overflow != 0 or counts beyond the host's bounds */
    uint32_t reserved;
} xrit_canvas_summary;               /* 168 bytes */

/* slots 1 .. 64, slot_bytes a multiple of 16 (> 0): slots * slot_bytes of pixel memory, allocated once, all zero.
 * No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_canvas_create(xrit_canvas **cv, int device, unsigned slots, size_t slot_bytes);
int xrit_canvas_destroy(xrit_canvas *cv);
/* everything zero, the pixels included; waits for the handle's last call */
int xrit_canvas_reset(xrit_canvas *cv);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_images_process_device.  d_bytes (n_bytes), d_pieces (max_pieces_in), d_files (max_files_in) and
 * d_files_summary are the files call's; d_image_bytes (n_image_bytes), d_lines (max_lines_in), d_image_files
 * (max_files_in) and d_images_summary the images call's.  If either summary has overflow != 0 or counts beyond these
 * bounds, only d_summary is written, with overflow = 2, and the state is unchanged.  d_canvas_files has max_files_in
 * entries, d_slots (the slot table after the call) as many as the handle has slots.  Every pointer but the two byte
 * buffers 8-byte aligned; d_image_bytes 4-byte aligned.  Calls on one handle share its state and scratch: keep them in
 * order. */
int xrit_canvas_process_device(xrit_canvas *cv, const uint8_t *d_bytes, size_t n_bytes, const xrit_file_piece *d_pieces,
                               size_t max_pieces_in, const xrit_file_record *d_files, size_t max_files_in,
                               const xrit_files_summary *d_files_summary, const uint8_t *d_image_bytes, size_t n_image_bytes,
                               const xrit_image_line *d_lines, size_t max_lines_in, const xrit_image_file *d_image_files,
                               const xrit_images_summary *d_images_summary, xrit_canvas_file *d_canvas_files,
                               xrit_canvas_slot *d_slots, xrit_canvas_summary *d_summary, void *stream);
/* host buffers (one upload, one download): what xrit_files_process and xrit_images_process returned; the n_* are the
 * lengths of the arrays handed over (the device's bounds).  canvas_files has n_files_in entries, slots as many as the
 * handle has.  XRIT_E_ARG with summary->overflow = 2 when the call was refused (nothing else written). */
int xrit_canvas_process(xrit_canvas *cv, const uint8_t *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t n_pieces_in,
                        const xrit_file_record *files, size_t n_files_in, const xrit_files_summary *files_summary,
                        const uint8_t *image_bytes, size_t n_image_bytes, const xrit_image_line *lines, size_t n_lines_in,
                        const xrit_image_file *image_files, const xrit_images_summary *images_summary,
                        xrit_canvas_file *canvas_files, xrit_canvas_slot *slots, xrit_canvas_summary *summary);
/* the first n_bytes (<= slot_bytes) of the slot's pixels -- a canvas is its first pitch * max_row -- to device memory,
 * queued on `stream` behind nothing: the caller orders it behind the handle's last call */
int xrit_canvas_read_device(xrit_canvas *cv, unsigned slot, uint8_t *d_out, size_t n_bytes, void *stream);
/* the slot's record and its pitch * max_row bytes after the handle's last call (waits for it); XRIT_E_CAPACITY, with
 * *info written, when max_bytes is less */
int xrit_canvas_read(xrit_canvas *cv, unsigned slot, uint8_t *out, size_t max_bytes, xrit_canvas_slot *info);
/* the slot's 64 segments after the handle's last call (waits for it) */
int xrit_canvas_segments(xrit_canvas *cv, unsigned slot, xrit_canvas_segment *out);
/* what key (vcid < 64, apid < 2048) carries after the handle's last call (waits for it) */
int xrit_canvas_key(xrit_canvas *cv, unsigned vcid, unsigned apid, xrit_canvas_key_state *out);
/* the counters after the handle's last call (waits for it) */
int xrit_canvas_stats(xrit_canvas *cv, xrit_canvas_counters *out);
/* the slot free again: pixels, record and segments zero, generation + 1 (so a file still open on it stops being
 * placed).  Queued on the stream of the handle's last call; no host synchronisation. */
int xrit_canvas_release(xrit_canvas *cv, unsigned slot);
/* the base of the slot's pixels in device memory (a canvas is its first pitch * max_row bytes), so that a stage behind
 * (xrit_product_process_device) reads a canvas in place.  Nothing is queued and nothing waited for: the caller orders
 * what reads the pixels behind the handle's last call, as with xrit_canvas_read_device. */
int xrit_canvas_pixels_device(xrit_canvas *cv, unsigned slot, const uint8_t **d_pixels);

/* ------------------------------------------------------------------------
 * Image products: what a ground station shows of an image -- a histogram, a
 * tone curve from it, the toned 8-bit image, a thumbnail that ignores missing
 * rows, and a two-channel false-colour composite -- made on the device from
 * pixels that are already there, a canvas slot above all (DESIGN.md section 23;
 * tests/product_spec.py is the specification).  Integer arithmetic throughout:
 * the device equals the specification byte for byte.
 *
 *  - an image (xrit_product_image): `rows` rows of `columns` samples of `bits`
 *    (1 .. 16) bits, `pitch` bytes from row to row; a sample is one byte for
 *    bits <= 8 and a little-endian uint16 above, as the image and canvas stages
 *    write them.  pitch >= columns * width; for width 2 pitch is even and d_pixels
 *    2-byte aligned; no other alignment is asked for.  columns, rows >= 1 and
 *    columns * rows <= 2^31.  Bytes of a row behind columns * width are never read.
 *  - a sample above 2^bits - 1 is taken as 2^bits - 1 (for the bin and for the tone
 *    table) and counted in out_of_range.  Value 0 is "no data": a free canvas is
 *    all zero, so rows of missing segments are zeros.
 *  - histogram: hist[v], uint32, 2^bits entries, over rows x columns.  With
 *    c[v] = hist[1] + .. + hist[v] and N = c[2^bits - 1]: min_nz and max_nz are the
 *    smallest and the largest v >= 1 with a count (0 if none).
 *  - tone table, 2^bits bytes, by params.tone:
 *      LINEAR    v >> (bits - 8) for bits >= 8, else v << (8 - bits).
 *      TABLE     the caller's d_table_in (2^bits bytes), copied.
 *      EQUALISE  lut[0] = 0; with cmin = c[min_nz], D = N - cmin: lut[v] = 1 for
 *                1 <= v < min_nz, 1 + (254 * (c[v] - cmin) + D / 2) / D from min_nz on
 *                (64-bit): data on 1 .. 255, no data stays 0.
 *      STRETCH   p_lo, p_hi per myriad, 0 <= p_lo < p_hi <= 10000: lo the smallest
 *                v >= 1 with c[v] > 0 and 10000 * c[v] >= p_lo * N, hi the smallest
 *                v >= 1 with 10000 * c[v] >= p_hi * N; lut[0] = 0, lut[v] = 1 for
 *                v <= lo, 255 for v >= hi, else
 *                1 + (254 * (v - lo) + (hi - lo) / 2) / (hi - lo).
 *    EQUALISE with D == 0, STRETCH with N == 0 or hi <= lo: LINEAR instead, and
 *    summary.fallback = 1.  lo and hi are in the summary: 0 where no STRETCH
 *    table was made.
 *  - toned image: rows x columns bytes, tight: lut[v].
 *  - thumbnail, params.factor f = 1 .. 64 (0: none): ceil(rows / f) x
 *    ceil(columns / f) bytes, tight.  Over the part of each f x f block inside the
 *    image, cnt the pixels with v != 0 and sum the sum of their lut[v]: the byte is
 *    0 for cnt == 0, else (2 * sum + cnt) / (2 * cnt).  Missing rows do not darken
 *    their neighbours.
 *  - composite: two toned 8-bit images of one size and the caller's table of
 *    256 x 256 x 3 bytes: rgb[y][x][k] = table[(a * 256 + b) * 3 + k], tight,
 *    interleaved (goesdump's false-colour lookup; no table is shipped).
 *  - the handle owns only scratch (a histogram, a tone table, a counter): no state
 *    between calls.  Calls on one handle share the scratch: keep them in order.
 * ------------------------------------------------------------------------ */
typedef struct xrit_product xrit_product;
#define XRIT_TONE_LINEAR    0
#define XRIT_TONE_TABLE     1
#define XRIT_TONE_EQUALISE  2
#define XRIT_TONE_STRETCH   3
#define XRIT_PRODUCT_MAX_FACTOR 64
typedef struct xrit_product_image {
    const uint8_t *d_pixels;         /* device memory (host memory for xrit_product_process) */
    uint32_t columns, rows, pitch, bits;
} xrit_product_image;                /* 24 bytes */
typedef struct xrit_product_params {
    uint32_t tone;                   /* XRIT_TONE_* */
    uint32_t p_lo, p_hi;             /* STRETCH: per myriad; ignored otherwise */
    uint32_t factor;                 /* thumbnail: 0 (none) or 1 .. 64 */
} xrit_product_params;               /* 16 bytes */
typedef struct xrit_product_summary {
    uint64_t total;                  /* rows * columns */
    uint64_t zeros;                  /* hist[0] */
    uint64_t out_of_range;           /* samples above 2^bits - 1 (counted in the last bin) */
    uint32_t min_nz, max_nz;
    uint32_t lo, hi;
    uint32_t fallback;               /* 1: EQUALISE or STRETCH had nothing to work on, the table is LINEAR's */
    uint32_t tone;                   /* the tone asked for */
    uint32_t tone_columns, tone_rows;
    uint32_t small_columns, small_rows;      /* 0, 0 for factor 0 */
} xrit_product_summary;              /* 64 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_product_create(xrit_product **pr, int device);
int xrit_product_destroy(xrit_product *pr);
/* waits for the handle's last call; there is no state to clear */
int xrit_product_reset(xrit_product *pr);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_canvas_process_device.  Outputs: d_hist (2^bits uint32, 4-byte aligned), d_lut (2^bits bytes), d_tone
 * (rows x columns bytes), d_small (factor > 0: ceil(rows / f) x ceil(columns / f) bytes), d_summary (8-byte aligned);
 * each but d_summary may be NULL and is then not written.  d_table_in (2^bits bytes) is read for XRIT_TONE_TABLE only.
 * Anything outside the bounds above, TABLE without a table, p_lo >= p_hi or p_hi > 10000, factor > 64:
 * XRIT_E_INVALID, nothing queued, nothing written. */
int xrit_product_process_device(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params,
                                const uint8_t *d_table_in, uint32_t *d_hist, uint8_t *d_lut, uint8_t *d_tone, uint8_t *d_small,
                                xrit_product_summary *d_summary, void *stream);
/* host buffers (one upload, one download): image->d_pixels and every other pointer are host memory */
int xrit_product_process(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params,
                         const uint8_t *table_in, uint32_t *hist, uint8_t *lut, uint8_t *tone, uint8_t *small,
                         xrit_product_summary *summary);
/* the image in device memory where it lies (a canvas slot: xrit_canvas_pixels_device, once the canvas handle's last call
 * has finished), every other pointer host memory: nothing is uploaded but TABLE's table, only the outputs asked for
 * are downloaded.  Runs on the handle's own stream and waits. */
int xrit_product_process_resident(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params,
                                  const uint8_t *table_in, uint32_t *hist, uint8_t *lut, uint8_t *tone, uint8_t *small,
                                  xrit_product_summary *summary);
/* Where the handle's last xrit_product_process or xrit_product_process_resident left the toned image and the thumbnail in
 * device memory (tight rows; NULL for one that call did not make, and before any such call): for a stage that goes on
 * with them there, xrit_jpeg_encode_resident above all.  They stay until the handle's next host-buffer call.  Nothing is
 * queued and nothing waited for. */
int xrit_product_outputs_device(xrit_product *pr, const uint8_t **d_tone, const uint8_t **d_small);
/* d_a, d_b: 8-bit images of columns x rows (>= 1, columns * rows <= 2^31), pitch_a, pitch_b >= columns; d_table
 * 256 * 256 * 3 bytes; d_rgb rows x columns x 3 bytes.  Asynchronous on `stream`, no host synchronisation. */
int xrit_product_composite_device(xrit_product *pr, const uint8_t *d_a, uint32_t pitch_a, const uint8_t *d_b, uint32_t pitch_b,
                                  uint32_t columns, uint32_t rows, const uint8_t *d_table, uint8_t *d_rgb, void *stream);
/* host buffers */
int xrit_product_composite(xrit_product *pr, const uint8_t *a, uint32_t pitch_a, const uint8_t *b, uint32_t pitch_b, uint32_t columns,
                           uint32_t rows, const uint8_t *table, uint8_t *rgb);

/* ------------------------------------------------------------------------
 * Image projection: an image in the instrument's scan geometry -- a canvas slot
 * above all -- resampled onto a latitude / longitude grid on the device, so that
 * it can be laid over a map, cut by coordinates or tiled (DESIGN.md section 24;
 * tests/geo_spec.py is the specification, csrc/geo_rule.h the rule both the
 * kernels and the host check are built from).  The geometry is the normalised
 * geostationary projection of the CGMS LRIT/HRIT Global Specification, 4.4.3.2,
 * with its constants as double literals: H = 42164.0, RPOL = 6356.5838, 0.993243,
 * E2 = 0.00675701, K = 1.006803 (the squared ratio of the radii),
 * R2D = 57.29577951308232.  The device equals the specification byte for byte:
 * per pixel there is only + - * / sqrt floor in IEEE double, in the order written
 * below, without FMA and without reciprocal or rsqrt substitution, and two
 * arctangents stated as a fixed polynomial.
 *
 *  - navigation (xrit_geo_nav): cfac, lfac, coff, loff are the four integers of
 *    the image navigation record (header type 2), either sign of the factors;
 *    origin is the number the first column and line carry (CGMS: 1);
 *    sub_lon_deg the sub-satellite longitude.
 *  - output grid: any cylindrical grid, as four tables of doubles in device
 *    memory that the handle holds.  Per output row i, with c_lat =
 *    atan(0.993243 * tan(lat_i)) and rl = RPOL / sqrt(1 - E2 * cos^2(c_lat)):
 *    A[i] = rl * cos(c_lat), B[i] = rl * sin(c_lat).  Per output column j:
 *    C[j] = cos(lon_j - sub_lon), S[j] = sin(lon_j - sub_lon).
 *    xrit_geo_set_grid makes them on the host with the C library (xrit_geo_grid_tables,
 *    which needs no device) and uploads them:
 *      XRIT_GEO_EQUIRECT  lon_j = lon0 + j * step_lon, lat_i = lat0 - i * step_lat
 *      XRIT_GEO_MERCATOR  the same longitudes; lat_i = atan(sinh(y0 - i * step_y)),
 *                         y0 and step_y being lat0_deg and step_lat_deg taken as
 *                         Mercator ordinates in radians
 *    columns and rows are 1 .. 16384.  xrit_geo_set_tables takes the caller's own.
 *  - the map, for output pixel (i, j):
 *      ac = A[i]*C[j];  r1 = H - ac;  r2 = -(A[i]*S[j]);  r3 = B[i]
 *      vis = r1 > 0 and H*ac >= r2*r2 + K*(r3*r3)
 *      u = -r2 / r1;    v = -r3 / sqrt(r1*r1 + r2*r2)
 *      x = atan_small(u) * R2D;   y = atan_small(v) * R2D
 *      fc = (double)(coff - origin) + x * ((double)cfac / 65536.0)
 *      fl = (double)(loff - origin) + y * ((double)lfac / 65536.0)
 *      qx = floor(fc*256.0 + 0.5);  qy = floor(fl*256.0 + 0.5)
 *    (qx, qy) is the source position in 1/256 pixel.  atan_small(t) = t * P(t*t), P
 *    the Horner form of sum_{k=0..9} (-1)^k / (2k+1) * z^k taken from k = 9 down,
 *    its coefficients the double literals 1.0 / (2k+1).  Visible points have
 *    |u|, |v| < 0.154; on |t| <= 0.2 the polynomial is within 1.2e-16 of atan.
 *    (r1 > 0 holds for every real table, ac being at most 6378.2: it is there so
 *    that a table holding +inf or 1e300 in C gives "off the disc" and not the
 *    sub-satellite pixel.)  A pixel that is not vis, or whose fc*256 or fl*256 is not below 2^30 in
 *    magnitude (NaN included), is off the disc: the map entry
 *    {INT32_MIN, INT32_MIN}.  That test stands in front of every index.
 *  - sampling: the source is an xrit_product_image (same layout and alignment
 *    rules); value 0 is "no data".  The output has the source's sample width,
 *    out_pitch bytes from row to row; bytes of a row behind columns * width are not
 *    written.
 *      XRIT_GEO_NEAREST   the sample at ((qx+128)>>8, (qy+128)>>8), 0 outside.
 *      XRIT_GEO_BILINEAR  x0 = qx>>8, fx = qx&255, y0 = qy>>8, fy = qy&255; the taps
 *                         (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) carry the
 *                         integer weights (256-fx | fx) * (256-fy | fy).  Taps
 *                         outside the image or of value 0 are left out.  W and V
 *                         the sums of weights and of weight * value over the taps
 *                         kept (64 bits): 0 for W = 0, else (2V + W) / (2W).  Data
 *                         never becomes 0 and missing rows do not darken their
 *                         neighbours: the thumbnail's rule.
 *    The summary counts total, off_disc, outside (visible, none of the taps -- the
 *    one of NEAREST, the four of BILINEAR whatever their weights -- inside the
 *    image), no_data (a tap inside, W = 0; NEAREST: the sample is 0) and written.
 *  - the handle owns the tables and the host-buffer forms' staging: no other state.
 *    Calls on one handle are kept in order.
 * ------------------------------------------------------------------------ */
typedef struct xrit_geo xrit_geo;
#define XRIT_GEO_EQUIRECT   0
#define XRIT_GEO_MERCATOR   1
#define XRIT_GEO_NEAREST    0
#define XRIT_GEO_BILINEAR   1
#define XRIT_GEO_MAX_DIM    16384
typedef struct xrit_geo_nav {
    int32_t cfac, lfac, coff, loff;
    int32_t origin;                  /* the number of the first column and line: CGMS says 1 */
    int32_t reserved;
    double  sub_lon_deg;
} xrit_geo_nav;                      /* 32 bytes */
typedef struct xrit_geo_grid {
    uint32_t kind;                   /* XRIT_GEO_EQUIRECT, XRIT_GEO_MERCATOR */
    uint32_t columns, rows;
    uint32_t reserved;
    double   lon0_deg, lat0_deg, step_lon_deg, step_lat_deg;
} xrit_geo_grid;                     /* 48 bytes */
typedef struct xrit_geo_point {
    int32_t qx, qy;                  /* 1/256 pixel; both INT32_MIN: off the disc */
} xrit_geo_point;                    /* 8 bytes */
typedef struct xrit_geo_summary {
    uint64_t total;                  /* rows * columns of the grid */
    uint64_t off_disc, outside, no_data, written;   /* they add up to total */
    uint32_t columns, rows;          /* the grid's */
    uint32_t width;                  /* bytes per sample */
    uint32_t mode;
} xrit_geo_summary;                  /* 56 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_geo_create(xrit_geo **g, int device);
int xrit_geo_destroy(xrit_geo *g);
/* waits for the handle's last call; the tables stay */
int xrit_geo_reset(xrit_geo *g);
/* the four tables of a grid, made on the host with the C library: A, B of grid->rows doubles, C, S of grid->columns.
 * Pure host code, never touches a device.  kind above 1, columns or rows outside 1 .. 16384: XRIT_E_INVALID. */
int xrit_geo_grid_tables(const xrit_geo_grid *grid, double sub_lon_deg, double *A, double *B, double *C, double *S);
/* xrit_geo_grid_tables, uploaded.  Waits for the handle's last call and for the upload: once per geometry. */
int xrit_geo_set_grid(xrit_geo *g, const xrit_geo_grid *grid, double sub_lon_deg);
/* the caller's own tables (host memory), whatever they hold; waits likewise */
int xrit_geo_set_tables(xrit_geo *g, uint32_t columns, uint32_t rows, const double *A, const double *B, const double *C, const double *S);
/* the tables in effect, read back from the device (waits); *columns, *rows: the grid's.  A table pointer may be NULL.
 * No tables set: XRIT_E_INVALID. */
int xrit_geo_tables(xrit_geo *g, uint32_t *columns, uint32_t *rows, double *A, double *B, double *C, double *S);
/* The calls below are asynchronous on `stream` (0: the null stream) with no host synchronisation.  No tables set, a mode
 * other than the two, an image outside the bounds of "Image products", out_pitch below columns * width or odd for
 * two-byte samples (d_out likewise), a NULL pointer, d_map not 8-byte aligned, d_summary not 8-byte aligned:
 * XRIT_E_INVALID, nothing queued, nothing written. */
/* the map of the grid: rows x columns entries, tight */
int xrit_geo_map_device(xrit_geo *g, const xrit_geo_nav *nav, xrit_geo_point *d_map, void *stream);
/* a map applied to an image: one geometry, many channels.  The entries may hold anything; nothing outside the image is
 * read. */
int xrit_geo_resample_device(xrit_geo *g, const xrit_product_image *image, const xrit_geo_point *d_map, uint32_t mode, uint8_t *d_out,
                             uint32_t out_pitch, xrit_geo_summary *d_summary, void *stream);
/* fused: the map is never stored; the output and the summary are those of map-then-resample byte for byte.  It may be
 * queued directly behind xrit_canvas_process_device on a slot's xrit_canvas_pixels_device. */
int xrit_geo_project_device(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *d_out,
                            uint32_t out_pitch, xrit_geo_summary *d_summary, void *stream);
/* host buffers (one upload, one download): image->d_pixels, out and summary are host memory */
int xrit_geo_project(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *out, uint32_t out_pitch,
                     xrit_geo_summary *summary);
/* the image in device memory where it lies, out and summary host memory.  Runs on the handle's own stream and waits. */
int xrit_geo_project_resident(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *out,
                              uint32_t out_pitch, xrit_geo_summary *summary);
/* Host helpers: plain C++, never touch a device. */
/* A file's header records (the primary header first), walked as the file stage walks them for the first record of type 2
 * and length 51: 32 bytes of projection name, then big-endian int32 CFAC, LFAC, COFF, LOFF.  The name must begin
 * "GEOS(" or "geos("; sub_lon_deg is the number between the parentheses; origin = 1.  Anything else (no such record, a
 * truncated header, another name, no number): XRIT_E_INVALID.  UNVERIFIED, our reading of the CGMS document, no recorded
 * downlink at hand: that layout, and that the name carries the longitude as a plain decimal number. */
int xrit_geo_parse_navigation(const uint8_t *header_bytes, size_t n, xrit_geo_nav *nav);
/* the inverse of the map (CGMS 4.4.3.2), with the C library, for choosing a grid: the longitude and latitude of the
 * point that (column, line), numbered from nav->origin, looks at.  Returns 0, 1 when it looks at space (nothing
 * written), or XRIT_E_INVALID. */
int xrit_geo_pixel_to_lonlat(const xrit_geo_nav *nav, double column, double line, double *lon_deg, double *lat_deg);

/* ------------------------------------------------------------------------
 * Map overlay: coastlines, borders and a latitude / longitude graticule drawn
 * into an image where it lies in device memory -- a toned view, a projected
 * image -- so that a cloud field can be placed by eye (DESIGN.md section 28;
 * tests/overlay_spec.py is the specification, csrc/overlay_rule.h the rules the
 * kernels and the host check are built from).  Polylines become a mask of one
 * byte per pixel, the mask is blended into the image.  Integer arithmetic from
 * the vertices on: the device equals the specification byte for byte, whatever
 * the order in which the segments are taken.
 *
 *  - vertices: an array of xrit_geo_point, qx, qy in 1/256 pixel of the target
 *    image, pixel centres at multiples of 256.  Segment i joins vertex i and
 *    i + 1 iff neither is a break.  A break is {INT32_MIN, INT32_MIN}; a vertex
 *    with |qx| or |qy| at or above 2^29 counts as one.  That keeps every product
 *    below in 64 bits, and this test stands in front of every index.
 *  - vertex map, scan geometry (xrit_overlay_map_device): per vertex a quad of
 *    doubles {A, B, C, S} as "Image projection" defines them for a row and a column;
 *    the point is that section's map entry, computed by the same function.  Off
 *    the disc, or a quad holding NaN: a break.  xrit_overlay_quads makes the quads
 *    of longitudes and latitudes on the host; xrit_overlay_grid_points gives the
 *    positions on an xrit_geo_grid directly.
 *  - the mask: rows x mask_pitch bytes, bit k of a byte: layer k (0 .. 7) drew
 *    here.  mask_pitch >= columns and a multiple of 4, d_mask 4-byte aligned;
 *    columns, rows 1 .. 16384.  Bits are set with 32-bit atomic OR, so a call adds
 *    to what is there, and calls on different layers may run in any order.
 *  - a segment with ends (x0, y0), (x1, y1), in exact integers:
 *      1. max_jump != 0 and |x1-x0| > max_jump or |y1-y0| > max_jump: not drawn,
 *         counted in `jumps` (the line across the picture where a grid wraps).
 *      2. Both end pixels ((x+128)>>8, (y+128)>>8) are stamped.
 *      3. The major axis is x iff |dx| >= |dy|; a the major, b the minor
 *         coordinate, the ends ordered so that a0 <= a1.
 *      4. a0 == a1: nothing more.
 *      5. For every integer m with a0 <= 256 m <= a1:
 *         minor = b0 + floor((2 (256 m - a0)(b1 - b0) + (a1 - a0)) / (2 (a1 - a0))),
 *         and pixel (m, (minor+128)>>8) (major, minor) is stamped.
 *      6. Before anything is walked the range of m is cut to
 *         -floor(w/2) .. dim - 1 + floor((w-1)/2), dim being the image's size along
 *         the major axis: the m whose stamp can reach the image along that axis.  A
 *         segment costs at most dim + w + 1 steps whatever its coordinates.
 *      7. A stamp of width w (1 .. 8) at (px, py) sets the pixels with offsets
 *         -floor((w-1)/2) .. floor(w/2) in both directions that lie inside the image.
 *  - the draw's summary: vertices = n; segments: pairs with both ends present;
 *    hidden: pairs with a break (segments + hidden = n - 1); jumps; drawn =
 *    segments - jumps; outside: drawn, but no stamp touched the image; steps: for
 *    every drawn segment 2 (the end stamps, wherever they fall) plus the number
 *    of m left after the cut of rule 6 (0 for a0 == a1).
 *  - two forms of the draw (xrit_overlay_set_form), the same mask and summary bit
 *    for bit: 0, a lane per segment walks its steps; 1 (a new handle's), the steps
 *    of all segments are counted and prefix-summed, and a lane takes one step.
 *  - blend: per pixel, k the highest set bit of the mask byte.  No bit: the
 *    output is the source (grey replicated for 1 -> 3 components).  Otherwise per
 *    channel out = (src * (255 - alpha_k) + c_k * alpha_k + 127) / 255, integer
 *    division, c = r, g, b of styles[k]; a one-component output uses
 *    c = (77 r + 150 g + 29 b + 128) >> 8.  The image is an xrit_product_image with
 *    bits == 8 and components_in (1 or 3, interleaved) bytes per pixel,
 *    pitch >= columns * components_in; components_out is 1 or 3, three in needs
 *    three out; out_pitch >= columns * components_out; mask_pitch >= columns; no
 *    alignment is asked for.  In place (d_out == image->d_pixels) is allowed when
 *    components and pitches are equal: every pixel is read and written by one
 *    lane.  Bytes of an output row behind columns * components_out are not written.
 *  - the handle owns scratch (8 bytes per vertex for form 1, the host-buffer
 *    forms' staging) and the form: no state between calls.  Calls on one handle
 *    share the scratch: keep them in order.  Once the scratch has its size no
 *    call synchronises with the host.
 * ------------------------------------------------------------------------ */
typedef struct xrit_overlay xrit_overlay;
#define XRIT_OVERLAY_MAX_DIM       16384
#define XRIT_OVERLAY_MAX_WIDTH     8
#define XRIT_OVERLAY_LAYERS        8
#define XRIT_OVERLAY_MAX_VERTICES  (1u << 26)
typedef struct xrit_overlay_style {
    uint8_t r, g, b, alpha;
} xrit_overlay_style;                /* 4 bytes */
typedef struct xrit_overlay_draw_summary {
    uint64_t vertices, segments, hidden, jumps, outside, drawn, steps;
    uint32_t layer, width;
} xrit_overlay_draw_summary;         /* 64 bytes */
typedef struct xrit_overlay_blend_summary {
    uint64_t pixels;                 /* rows * columns */
    uint64_t covered;                /* pixels with a mask bit */
    uint64_t by_layer[8];            /* of those, by their top layer: they add up to covered */
    uint32_t columns, rows, components_in, components_out;
} xrit_overlay_blend_summary;        /* 96 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path".  A new handle has form 1. */
int xrit_overlay_create(xrit_overlay **ov, int device);
int xrit_overlay_destroy(xrit_overlay *ov);
/* waits for the handle's last call; there is no state to clear */
int xrit_overlay_reset(xrit_overlay *ov);
/* form 0 or 1; anything else XRIT_E_INVALID, nothing changed */
int xrit_overlay_set_form(xrit_overlay *ov, uint32_t form);
/* The _device calls are asynchronous on `stream` (0: the null stream).  A NULL pointer (n == 0 allows NULL vertices),
 * n above 2^26, layer > 7, width 0 or above 8, columns or rows outside 1 .. 16384, a pitch too small, mask_pitch or
 * d_mask not a multiple of 4 (draw), d_quads, d_points or a summary not 8-byte aligned, an image outside the bounds above:
 * XRIT_E_INVALID, nothing queued, nothing written. */
/* n quads {A, B, C, S} -> n points */
int xrit_overlay_map_device(xrit_overlay *ov, const xrit_geo_nav *nav, const double *d_quads, size_t n, xrit_geo_point *d_points, void *stream);
/* clear != 0: rows * mask_pitch bytes of the mask are zeroed first */
int xrit_overlay_draw_device(xrit_overlay *ov, const xrit_geo_point *d_points, size_t n, uint32_t layer, uint32_t width, uint32_t max_jump,
                             uint8_t *d_mask, uint32_t columns, uint32_t rows, uint32_t mask_pitch, uint32_t clear,
                             xrit_overlay_draw_summary *d_summary, void *stream);
/* styles: XRIT_OVERLAY_LAYERS entries in host memory, copied into the launch */
int xrit_overlay_blend_device(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *d_mask,
                              uint32_t mask_pitch, const xrit_overlay_style *styles, uint8_t *d_out, uint32_t out_pitch,
                              uint32_t components_out, xrit_overlay_blend_summary *d_summary, void *stream);
/* host buffers (one upload, one download; run on the handle's own stream and wait): every pointer is host memory.  The
 * draw uploads the mask unless clear != 0. */
int xrit_overlay_map(xrit_overlay *ov, const xrit_geo_nav *nav, const double *quads, size_t n, xrit_geo_point *points);
int xrit_overlay_draw(xrit_overlay *ov, const xrit_geo_point *points, size_t n, uint32_t layer, uint32_t width, uint32_t max_jump,
                      uint8_t *mask, uint32_t columns, uint32_t rows, uint32_t mask_pitch, uint32_t clear, xrit_overlay_draw_summary *summary);
int xrit_overlay_blend(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *mask, uint32_t mask_pitch,
                       const xrit_overlay_style *styles, uint8_t *out, uint32_t out_pitch, uint32_t components_out,
                       xrit_overlay_blend_summary *summary);
/* the image and the mask in device memory where they lie (a toned view behind xrit_product_outputs_device, a mask drawn by
 * xrit_overlay_draw_device), out and summary host memory */
int xrit_overlay_blend_resident(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *d_mask,
                                uint32_t mask_pitch, const xrit_overlay_style *styles, uint8_t *out, uint32_t out_pitch,
                                uint32_t components_out, xrit_overlay_blend_summary *summary);
/* Where the handle's last xrit_overlay_draw left the mask in device memory (rows x mask_pitch bytes as that call was
 * given them; NULL before any such call): for xrit_overlay_blend_resident behind it.  It stays until the handle's next
 * xrit_overlay_draw.  Nothing is queued and nothing waited for. */
int xrit_overlay_mask_device(xrit_overlay *ov, const uint8_t **d_mask);
/* Host helpers: plain C++ on the C library, never touch a device.  In longitude / latitude arrays a vertex with NaN in
 * either coordinate is a break. */
/* the quads of n vertices, by the formulas of xrit_geo_grid_tables per vertex; NaN in either coordinate: a NaN quad */
int xrit_overlay_quads(const double *lon_deg, const double *lat_deg, size_t n, double sub_lon_deg, double *quads);
/* the positions on a grid in 1/256 pixel: column (d / step_lon) with d = lon - lon0 brought into [-180, 180), row
 * (lat0 - lat) / step_lat, for XRIT_GEO_MERCATOR (lat0 - asinh(tan(lat))) / step_lat; q = floor(256 v + 0.5).  NaN, or a
 * position not below 2^29 in magnitude: a break. */
int xrit_overlay_grid_points(const xrit_geo_grid *grid, const double *lon_deg, const double *lat_deg, size_t n, xrit_geo_point *points);
/* a segment longer than max_step_deg in either coordinate is split into k = ceil(max(|dlon|, |dlat|) / max_step_deg)
 * equal parts in lon / lat (vertex j of them: p0 + (p1 - p0) * j / k); breaks are kept.  *n_out: the vertices this makes;
 * XRIT_E_CAPACITY (and the true *n_out, the first cap written) when cap is too small; more than 2^26: XRIT_E_INVALID. */
int xrit_overlay_densify(const double *lon_deg, const double *lat_deg, size_t n, double max_step_deg, double *out_lon, double *out_lat,
                         size_t cap, size_t *n_out);
/* meridians at -180 + i * step_deg below 180, from latitude -90 to 90, then parallels at -90 + i * step_deg strictly
 * between the poles, from longitude -180 to 180, each with a vertex every vertex_step_deg (the last one on the end) and a
 * break behind it.  step_deg 0.1 .. 90, vertex_step_deg 0.001 .. step_deg; steps that make more than 2^26 vertices:
 * XRIT_E_INVALID, decided from the steps before anything is written.  *n_out and XRIT_E_CAPACITY as above. */
int xrit_overlay_graticule(double step_deg, double vertex_step_deg, double *lon_deg, double *lat_deg, size_t cap, size_t *n_out);

/* ------------------------------------------------------------------------
 * JPEG: an 8-bit image in device memory -- the product stage's toned image,
 * its thumbnail, its composite, a projected image -- becomes a complete
 * baseline JFIF file in device memory, so that only the file's bytes cross to
 * the host (tests/jpeg_spec.py is the specification).
 * The file is the one libjpeg writes for the same pixels and parameters: the
 * device equals the specification byte for byte, and so does Pillow's libjpeg.
 *
 *  - input: `rows` rows of `columns` pixels, `pitch` bytes from row to row.  One
 *    component: one byte per pixel, pitch >= columns.  Three: interleaved R, G, B
 *    as xrit_product_composite_device writes them, pitch >= 3 * columns.
 *    1 <= columns, rows <= 65535; no alignment is asked of d_pixels or pitch;
 *    bytes of a row behind the image are never read.  (The bits field of
 *    xrit_product_image is ignored.)
 *  - the stage takes at most XRIT_JPEG_MAX_BLOCKS (2^22) 8 x 8 blocks of all
 *    components in one call: ceil(columns / 8) * ceil(rows / 8) * components.  A
 *    larger shape is XRIT_E_INVALID and xrit_jpeg_bound is 0 for it.  (The scratch
 *    holds 400 bytes per block; inside the stage bit and byte offsets are 64 and
 *    32 bits wide, and 2^22 blocks stay below 2^32 bytes at 208 bytes a block.)
 *  - quantisation: either quality 1 .. 100, libjpeg's scaling of the Annex K
 *    tables (s = 5000 / q below 50, else 200 - 2 q; entry (base * s + 50) / 100,
 *    clamped to 1 .. 255), or the caller's two tables of 64 bytes in natural
 *    (row-major) order, entries 1 .. 255.  One component uses table 0 only.
 *  - restart, in MCUs: 0 none; 1 .. 65535 a DRI segment and RSTm between the
 *    intervals, m counting modulo 8.
 *  - colour: libjpeg's 16-bit fixed point RGB -> YCbCr, 4:4:4; an MCU is the Y,
 *    Cb, Cr blocks of one 8 x 8 position.  Y: table 0 and the luminance Huffman
 *    tables; Cb, Cr: table 1 and the chrominance ones.
 *  - blocks: the image padded to multiples of 8 by repeating the last column,
 *    then the last row; 128 subtracted; jfdctint (13-bit constants, PASS1_BITS
 *    2, rows then columns); with qv = q << 3 the level (|c| + (qv >> 1)) / qv,
 *    sign restored.
 *  - entropy code: baseline Huffman, the Annex K tables as they stand; the DC
 *    predictor is zero at every restart; ZRL for runs above 15, EOB unless
 *    coefficient 63 is non-zero.  Most significant bit first, every 0xFF data
 *    byte followed by 0x00, the last byte in front of a marker filled with
 *    1-bits (and stuffed if that makes it 0xFF).
 *  - the file: SOI, APP0 (JFIF 1.01, no density), DQT per table, SOF0, one DHT
 *    per table, DRI if restart > 0, SOS, the scan, EOI.
 *  - d_result (xrit_jpeg_result, 8-byte aligned): size is the file's length
 *    whether or not it fitted, status 1 if size > cap.  No byte at or behind
 *    d_out + cap is ever written; with status 1 the bytes in front are unspecified.
 *  - the bound of a file (xrit_jpeg_bound): a block is at most 22 + 63 * 26 bits
 *    (the longest DC code, 11 bits in the chrominance table -- the luminance
 *    table's longest has 9 -- and 11 magnitude bits, 63 times a 16-bit code and 10
 *    bits); an interval's bits are rounded up to a byte; every byte may be 0xFF
 *    and stuffed, which doubles it; 2 bytes of marker between intervals, the
 *    header and EOI on top:  header + 2 * (ceil(blocks * 1660 / 8) + intervals)
 *    + 2 * (intervals - 1) + 2.
 *  - the handle owns only scratch and the parameters: no state between calls.
 *    Calls on one handle share the scratch: keep them in order.
 * ------------------------------------------------------------------------ */
typedef struct xrit_jpeg xrit_jpeg;
#define XRIT_JPEG_MAX_BLOCKS (1u << 22)
typedef struct xrit_jpeg_result {
    uint64_t size;                   /* the file's length */
    uint32_t status;                 /* 1: size > cap, the file did not fit */
    uint32_t restarts;               /* restart markers in the file */
} xrit_jpeg_result;                  /* 16 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path".  A new handle has quality 90, restart 0. */
int xrit_jpeg_create(xrit_jpeg **j, int device);
int xrit_jpeg_destroy(xrit_jpeg *j);
/* waits for the handle's last call; the parameters stay */
int xrit_jpeg_reset(xrit_jpeg *j);
/* quality 1 .. 100, restart 0 .. 65535; anything else XRIT_E_INVALID, nothing changed */
int xrit_jpeg_set_quality(xrit_jpeg *j, uint32_t quality, uint32_t restart);
/* tables128: table 0 then table 1, natural order, every entry 1 .. 255 */
int xrit_jpeg_set_tables(xrit_jpeg *j, const uint8_t *tables128, uint32_t restart);
/* Host only, no device is touched: the bytes SOI .. SOS that the device will write for that shape with the handle's
 * parameters.  *n is their number; they are written to out when n <= cap (out may be NULL with cap 0). */
int xrit_jpeg_header(const xrit_jpeg *j, uint32_t components, uint32_t columns, uint32_t rows, uint8_t *out, size_t cap, size_t *n);
/* Host only, without a handle: the two tables that xrit_jpeg_set_quality selects (128 bytes, natural order), and the
 * header for given tables and restart. */
int xrit_jpeg_quality_tables(uint32_t quality, uint8_t *tables128);
int xrit_jpeg_header_for(const uint8_t *tables128, uint32_t restart, uint32_t components, uint32_t columns, uint32_t rows, uint8_t *out,
                         size_t cap, size_t *n);
/* Host only: the largest file any input of that shape can produce (the derivation is above); 0 for a shape or a restart
 * that the stage refuses. */
uint64_t xrit_jpeg_bound(uint32_t components, uint32_t columns, uint32_t rows, uint32_t restart);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation: it may be queued directly
 * behind xrit_product_process_device, xrit_product_composite_device and xrit_geo_*.  components 1 or 3.  Components
 * other than 1 or 3, a zero or too large dimension, a pitch too small, a NULL d_out or d_result (cap = 0 too):
 * XRIT_E_INVALID, nothing queued, nothing written. */
int xrit_jpeg_encode_device(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *d_out, size_t cap,
                            xrit_jpeg_result *d_result, void *stream);
/* host buffers (one upload, one download of min(size, cap) bytes): image->d_pixels, out and result are host memory.
 * XRIT_E_CAPACITY when the file did not fit (result says how long it is). */
int xrit_jpeg_encode(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *out, size_t cap, xrit_jpeg_result *result);
/* the pixels in device memory where they lie, out and result host memory: nothing is uploaded, only the file's bytes are
 * downloaded.  Runs on the handle's own stream and waits. */
int xrit_jpeg_encode_resident(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *out, size_t cap,
                              xrit_jpeg_result *result);

/* ------------------------------------------------------------------------
 * JPEG decoder: a batch of baseline JPEG streams in device memory -> the
 * pixels libjpeg gives for them (tests/jpegdec_spec.py
 * is the specification).  The data field of an LRIT/HRIT image file whose
 * image structure record has compression flag 2 is such a stream.
 *
 *  - input: the streams lie in one byte buffer; each is named by a record
 *    that begins {uint64 offset; uint32 length}, `stride` bytes apart (a
 *    multiple of 4, at least 12), as for xrit_rice_decode_device: an
 *    xrit_file_piece or a record of the caller's.  A record that reaches
 *    outside the buffer is XRIT_JPEGDEC_DAMAGED.
 *  - accepted: baseline sequential DCT (SOF0), 8-bit samples; one component,
 *    or three components all sampled 1 x 1, taken as YCbCr; any DQT with 8-bit
 *    entries in any of the four slots; any DHT in any of the four slots whose
 *    DC symbols are 0 .. 11 and whose AC symbols have a size of 0 .. 10; DRI
 *    of any value with RSTm markers; APPn, COM and other segments with a
 *    length are skipped; bytes behind EOI are ignored, a missing EOI too.
 *  - output: the pixels of every image back to back in item order, rows tight
 *    (columns * components bytes; three components: interleaved RGB through
 *    libjpeg's fixed-point YCbCr -> RGB), each image padded with zeros to a
 *    multiple of 4 bytes; one xrit_jpegdec_record per item; one summary.
 *    An image is written iff offset + padded length <= cap; the summary has
 *    the true total and overflow = 1 otherwise.  An image with a non-zero
 *    status that has a geometry (the statuses from 4 on) takes its room and
 *    its pixel bytes are all zero; the others have length 0 and offset 0.
 *  - arithmetic: jidctint operation for operation (columns descaled by 11,
 *    rows by 18, 13-bit constants), samples clip(v + 128, 0, 255), in 32-bit
 *    two's complement; the DC predictor is kept in 16 bits.
 *  - the statuses are those of the SERIAL walk: the first thing wrong in the
 *    order header chain, then per restart interval its bits, then the marker
 *    behind it.
 *      0 OK
 *      1 UNSUPPORTED  a JPEG this stage does not decode: progressive, extended,
 *                     lossless or hierarchical SOF, arithmetic coding, 12-bit
 *                     samples, 16-bit quantiser entries, subsampled components,
 *                     2 or 4 and more components, a scan that does not name
 *                     every component (several scans)
 *      2 DAMAGED      the chain SOI .. SOS is broken: no SOI, a segment that
 *                     runs past `length`, no SOF in front of SOS, dimensions of
 *                     0, SOS naming a table never defined, a DHT that is no
 *                     prefix code or has symbols out of range
 *      3 TOO_LARGE    more than 2^22 blocks of 8 x 8 in the image; or the item
 *                     brings the call's running total of blocks above
 *                     max_blocks or of entropy-coded bytes above n_bytes (only
 *                     overlapping items can): it and every sound item behind it
 *      4 BAD_CODE     16 bits that begin no code
 *      5 INDEX        a coefficient index past 63
 *      6 SHORT        a restart interval out of bits before its MCUs
 *      7 INTERVALS    fewer or more restart intervals than the geometry asks for
 *      8 RST_ORDER    an RSTm out of sequence
 *      9 MARKER       a marker other than RSTm or EOI in the scan
 *    Damage never changes a neighbouring image.  No byte outside the buffers
 *    handed over is read or written for any input bytes whatever.
 *  - the handle owns only scratch and the form: no state between calls, so the
 *    stage queues in front of xrit_product_*, xrit_geo_* and xrit_jpeg_* on one
 *    stream; describe an image to them with an xrit_product_image {d_pixels +
 *    offset, columns, rows, pitch = columns * components, bits = 8}.
 * ------------------------------------------------------------------------ */
typedef struct xrit_jpegdec xrit_jpegdec;
#define XRIT_JPEGDEC_OK          0
#define XRIT_JPEGDEC_UNSUPPORTED 1
#define XRIT_JPEGDEC_DAMAGED     2
#define XRIT_JPEGDEC_TOO_LARGE   3
#define XRIT_JPEGDEC_BAD_CODE    4
#define XRIT_JPEGDEC_INDEX       5
#define XRIT_JPEGDEC_SHORT       6
#define XRIT_JPEGDEC_INTERVALS   7
#define XRIT_JPEGDEC_RST_ORDER   8
#define XRIT_JPEGDEC_MARKER      9
#define XRIT_JPEGDEC_STATUSES    10
#define XRIT_JPEGDEC_MAX_BLOCKS  (1u << 22)
#define XRIT_JPEGDEC_DEFAULT_BLOCKS (1u << 16)
#define XRIT_JPEGDEC_MAX_BYTES   (1u << 28)   /* n_bytes of one call */
#define XRIT_JPEGDEC_MAX_ITEMS   (1u << 20)
typedef struct xrit_jpegdec_record {
    uint64_t offset;                 /* of the image's pixels in the output */
    uint64_t length;                 /* columns * rows * components, without the padding */
    uint32_t columns, rows, components;
    uint32_t restart;                /* the DRI value */
    uint32_t intervals;              /* restart intervals found in the scan */
    uint32_t status;
    uint32_t reserved[6];
} xrit_jpegdec_record;               /* 64 bytes */
typedef struct xrit_jpegdec_summary {
    uint64_t images;                 /* items with status 0 */
    uint64_t bytes;                  /* pixel bytes of all items with their padding, whether or not they fitted */
    uint32_t by_status[XRIT_JPEGDEC_STATUSES];
    uint32_t overflow;               /* 1: an image did not fit below cap */
    uint32_t reserved;
} xrit_jpegdec_summary;              /* 64 bytes */
typedef struct xrit_jpegdec_info {
    uint32_t columns, rows, components, restart, status;
    uint32_t scan_offset;            /* the first byte behind SOS */
    uint32_t blocks, intervals;      /* what the geometry asks for */
} xrit_jpegdec_info;                 /* 32 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path".  A new handle has form 1 and subsequences of 1024 bits. */
int xrit_jpegdec_create(xrit_jpegdec **d, int device);
int xrit_jpegdec_destroy(xrit_jpegdec *d);
/* waits for the handle's last call; the form stays */
int xrit_jpegdec_reset(xrit_jpegdec *d);
/* The entropy decoder's form.  0: one lane per restart interval, the plain serial walk.  1: one wave per interval, the
 * interval cut into subsequences of subsequence_bits (32 .. 2^20, 0: 1024) that 64 lanes walk from guessed states until
 * the states are the serial walk's.  Both give the same coefficients bit for bit.  Anything else: XRIT_E_INVALID. */
int xrit_jpegdec_set_form(xrit_jpegdec *d, uint32_t form, uint32_t subsequence_bits);
/* Host only, no device is touched: the header chain of one stream in host memory -> its geometry and status (0, 1, 2 or 3),
 * so that a caller can size the output: an image takes columns * rows * components bytes rounded up to 4. */
int xrit_jpegdec_header(const uint8_t *data, size_t length, xrit_jpegdec_info *info);
/* device pointers, asynchronous on `stream` (0: the null stream); no host synchronisation once the scratch has its size for
 * (n_items, n_bytes, max_blocks).  max_blocks: the blocks of 8 x 8 of all components the call's scratch, grids and scans
 * are sized for (0: XRIT_JPEGDEC_DEFAULT_BLOCKS = 2^16, a 2048 x 2048 grey image; give the batch's own bound, from
 * xrit_jpegdec_header, for more).  The scratch costs about 132 bytes per block of max_blocks (128 of them the int16
 * coefficients: 8.6 MB at the default, 554 MB at 2^22), 3.5 bytes per byte of n_bytes and 5.6 KB per item.  NULL pointers (d_bytes, d_items with n_items 0 and d_pixels with cap 0 excepted), n_bytes above 2^28, n_items
 * above 2^20, max_blocks above 2^22, a stride below 12 or no multiple of 4, records or a summary that are not 8-byte
 * aligned: XRIT_E_INVALID, nothing queued, nothing written. */
int xrit_jpegdec_decode_device(xrit_jpegdec *d, const uint8_t *d_bytes, size_t n_bytes, const void *d_items, size_t stride, size_t n_items,
                               size_t max_blocks, uint8_t *d_pixels, size_t cap, xrit_jpegdec_record *d_records,
                               xrit_jpegdec_summary *d_summary, void *stream);
/* host buffers: the bytes and the records are uploaded, the scratch is sized from the headers (read on the host), the
 * summary and the records are downloaded, then the pixel bytes up to the end of the last image that fitted.
 * XRIT_E_CAPACITY when an image did not fit: the records are all there, the pixels of the images that fitted are written,
 * the room of one that did not is left as it was. */
int xrit_jpegdec_decode(xrit_jpegdec *d, const uint8_t *bytes, size_t n_bytes, const void *items, size_t stride, size_t n_items, uint8_t *pixels,
                        size_t cap, xrit_jpegdec_record *records, xrit_jpegdec_summary *summary);
/* after the handle's last call (waits for it): the most rounds a tile of 64 subsequences took in form 1 (0 in form 0) */
int xrit_jpegdec_rounds(xrit_jpegdec *d, uint32_t *rounds);

/* ------------------------------------------------------------------------
 * Carrier acquisition: a stage IN FRONT of the chain that finds a large carrier
 * offset and takes it out on the device (DESIGN.md section 21;
 * tests/acquire_spec.py is the specification).  The reference has no such
 * stage: its only tuning is the `frequency` key of the config file
 * (demodulator.cpp:285-290, :461), retuned by hand while watching the
 * constellation, and its Costas loop locks within about 0.7 kHz at 1.25 Msps.
 * Samples are converted as onSamplesAvailable does (demodulator.cpp:54-74):
 * XRIT_SAMPLE_FLOATIQ as is, S16IQ times 2^-15, S8IQ times 2^-7;
 * XRIT_SAMPLE_U8IQ is refused with XRIT_E_INVALID (its DC tracker belongs to the
 * chain's ingest).  The output is cf32 and goes to the chain as
 * XRIT_SAMPLE_FLOATIQ.
 *  - state, in device memory: acc (uint64, the oscillator's phase in units of
 *    2^-64 turn) and inc (int64, the phase step per input sample); both 0 after
 *    create and reset.
 *  - mix: sample i of a call, with a = acc + i * inc (mod 2^64):
 *      h = (int32)(a >> 32); theta = (float)h * (float)(pi * 2^-31);
 *      (s, c) = sincosf(theta)   -- the C library's, bit for bit;
 *      yr = xr * c + xi * s; yi = xi * c - xr * s   -- float32, no FMA;
 *    afterwards acc += n * inc.  The phase is an integer, so the output does not
 *    depend on how a stream is cut into calls, and a change of inc is a
 *    frequency step without a phase jump.
 *  - estimate: u[m] = the sum of pre_sum consecutive samples, z = u * u (BPSK
 *    squared: a spectral line at twice the carrier); M segments of N = 4096 points
 *    of z, half overlapped, Hann window, FFT; P[k] = the sum of the segments'
 *    |X_s[k]|^2, k0 its first maximum; the phase of sum_s X_s[k0] conj(X_{s-1}[k0])
 *    times (-1)^k0 places the line inside the bin.  M = min(segments,
 *    floor(floor(n / pre_sum) / 2048) - 1).  float32 through |X|^2, float64 behind
 *    it; no atomics: the same bits from run to run.
 *    A sample that is not finite, or whose square is not in float32, gives status
 *    WEAK whenever it lies within the samples the estimate reads, and is never
 *    applied; k0, ratio and nu are then unspecified but the same from run to run,
 *    and inc is 0 when nu is NaN.  Silence is WEAK too (ratio NaN, k0, nu and inc
 *    0).  Samples beyond (M + 1) * 2048 * pre_sum, and beyond the last whole
 *    pre-sum, are not read.
 *    UNAMBIGUOUS ONLY FOR |f| < sample_rate / (4 * pre_sum).
 *    A strong DC component squares to a line at 0 Hz and would be taken for the
 *    carrier; behaviour under adjacent-channel interference is not known
 *    ("Unverified").
 * ------------------------------------------------------------------------ */
typedef struct xrit_acquire xrit_acquire;
#define XRIT_ACQUIRE_OK        0
#define XRIT_ACQUIRE_TOO_SHORT 1     /* fewer than 31 segments: n < 65536 * pre_sum */
#define XRIT_ACQUIRE_WEAK      2     /* ratio < min_ratio: no line stands out */
typedef struct xrit_acquire_params {
    double   sample_rate;            /* Hz, > 0 */
    uint32_t pre_sum;                /* R: 1 .. 64; 0 selects 1 */
    uint32_t segments;               /* the most segments an estimate takes: 31 .. 4095; 0 selects 511 */
    double   min_ratio;              /* P[k0] / mean(P) below which the result is WEAK; 0 selects the default (8.9) */
} xrit_acquire_params;               /* 24 bytes */
typedef struct xrit_acquire_estimate_record {
    uint32_t status;                 /* XRIT_ACQUIRE_* */
    uint32_t k0;                     /* the line's bin in the squared signal's spectrum (0 when TOO_SHORT) */
    uint32_t segments;               /* M */
    uint32_t reserved0;
    double   ratio;                  /* P[k0] / mean(P) */
    double   nu;                     /* cycles per input sample, in [-1/(4R), 1/(4R)) */
    double   hz;                     /* nu * sample_rate */
    int64_t  inc;                    /* rint(ldexp(nu, 64)) */
    uint32_t applied;                /* 1: this call made it the state's inc */
    uint32_t reserved[3];
} xrit_acquire_estimate_record;      /* 64 bytes */
typedef struct xrit_acquire_state {
    uint64_t acc;
    int64_t  inc;
    uint64_t samples_mixed, estimates, applied;      /* since create or reset */
} xrit_acquire_state;                /* 40 bytes */

/* No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_acquire_create(xrit_acquire **aq, const xrit_acquire_params *params, int device);
int xrit_acquire_destroy(xrit_acquire *aq);
/* acc, inc and the counters zero; waits for the handle's last call */
int xrit_acquire_reset(xrit_acquire *aq);
/* inc = llrint(ldexp(hz / sample_rate, 64)), |hz| < sample_rate / 2; acc is untouched.  Queued on the stream of the
 * handle's last call; no host synchronisation. */
int xrit_acquire_set_frequency(xrit_acquire *aq, double hz);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation.  The estimate is of the n raw
 * samples at d_samples (aligned to one complex sample), never of mixed output.  d_record (8-byte aligned) is always
 * written.  apply != 0 and status OK: the state's inc becomes the record's.  Calls on one handle share its state and
 * scratch: keep them in order. */
int xrit_acquire_estimate_device(xrit_acquire *aq, const void *d_samples, size_t n_complex, int sample_type, int apply,
                                 xrit_acquire_estimate_record *d_record, void *stream);
/* d_out: n_complex cf32 (8-byte aligned); for XRIT_SAMPLE_FLOATIQ it may be d_samples itself.  16-byte loads and stores
 * when both pointers are 16-byte aligned.  n_complex = 0 is a call like any other.  May be queued directly behind
 * xrit_acquire_estimate_device and in front of xrit_demod_process_device on one stream. */
int xrit_acquire_mix_device(xrit_acquire *aq, const void *d_samples, size_t n_complex, int sample_type, float *d_out,
                            void *stream);
/* host buffers: one upload, one download each */
int xrit_acquire_estimate(xrit_acquire *aq, const void *samples, size_t n_complex, int sample_type, int apply,
                          xrit_acquire_estimate_record *record);
int xrit_acquire_mix(xrit_acquire *aq, const void *samples, size_t n_complex, int sample_type, float *out);
/* the state after the handle's last call (waits for it) */
int xrit_acquire_get_state(xrit_acquire *aq, xrit_acquire_state *out);

/* ------------------------------------------------------------------------
 * Link monitor: a stage BEHIND the chain that says how good the link was, and
 * when: per block of symbols the level, two Es/N0 estimates, how often the int8
 * sink saturates and how often the sign changes (DESIGN.md section 22;
 * tests/monitor_spec.py is the specification).  The reference shows a
 * constellation (DiagManager) and a "signal quality" figure in its decoder; a
 * recorded capture runs through this library far faster than anyone can watch,
 * so what is kept is a time series.
 *  - lattice: every symbol becomes an integer q.  XRIT_SYMBOL_F32:
 *      q = clamp(rintf(x * 512.0f), -4095, 4095)   -- the product is exact, rintf
 *    rounds to nearest even; NaN gives q = 0 and counts in `bad`; `clamped`
 *    counts |rintf(512 x)| > 4095, +-inf included.  XRIT_SYMBOL_I8: q = 4 * s
 *    (4 * 127 = 508: both types share the level scale to 1 %).
 *  - a block record holds sums over its n symbols: s1 = sum |q|, s2 = sum q^2,
 *    s4 = sum q^4, sum = sum q; sat = the symbols the int8 sink saturates
 *    (F32: |q| > 512, that is |x| > 1; I8: s = 127 or s = -128); neg = q < 0;
 *    flips = the symbols whose (q < 0) differs from that of the symbol before
 *    them in the stream -- across blocks and calls; the first symbol after
 *    create or reset counts none.  All integers: the sums do not depend on their
 *    order, and rows, summary and state are the specification's word for word
 *    however a stream is cut into calls.
 *  - block: a multiple of 64 in 64 .. 32768 (0 selects 16384, one coded frame);
 *    4095^4 * 32768 < 2^63, so s4 fits with a bit to spare.
 *  - state, in device memory, all zero after create and reset: the open block's
 *    partial record, the last symbol's sign and whether there is one, the totals,
 *    and a cumulative histogram hist[(q + 4096) >> 5] of every symbol pushed.
 * NO LOCK FLAG.  A carrier that is not locked reads 1.5 .. 2.5 dB from real
 * soft symbols (a spinning 8 dB carrier: 1.2 .. 2.5 dB), and a working LRIT link
 * can sit there too: the reading alone cannot tell the two apart.  Lock is the
 * frame lock's business (xrit_lock_*); what the monitor shows is the reading
 * against what the user expected.
 * ------------------------------------------------------------------------ */
typedef struct xrit_monitor xrit_monitor;
#define XRIT_SYMBOL_F32 0      /* the chain's soft symbols */
#define XRIT_SYMBOL_I8  1      /* xrit_quantize_i8's output, the TCP sink's bytes */
#define XRIT_MONITOR_NO_SIGNAL 1     /* 3 s2^2 - n s4 <= 0 (or s1 = 0): no signal power to be found; the dB value is -99 */
#define XRIT_MONITOR_NO_NOISE  2     /* a noise term <= 0 (every |q| the same): the dB value is +99 */
typedef struct xrit_monitor_block {
    uint64_t first;                  /* index in the stream of the block's first symbol */
    uint32_t n;                      /* symbols in it: the block size (less only in the state's open block) */
    uint32_t flips;
    uint64_t s1, s2, s4;             /* sums of |q|, q^2, q^4 */
    int64_t  sum;                    /* sum of q */
    uint32_t sat, clamped, bad, neg;
} xrit_monitor_block;                /* 64 bytes */
typedef struct xrit_monitor_summary {
    uint64_t rows;                   /* blocks this call completed and wrote */
    uint64_t open_n;                 /* symbols in the open block behind it */
    uint64_t symbols_total, blocks_total;
} xrit_monitor_summary;              /* 32 bytes */
typedef struct xrit_monitor_state {
    xrit_monitor_block open;
    uint64_t symbols_total, blocks_total, calls;
    uint32_t last_neg, have_last;
    uint64_t hist[256];
} xrit_monitor_state;                /* 2144 bytes */
typedef struct xrit_monitor_quality {
    double   level;                  /* sqrt(s2 / n) / 512 (I8: / 508): the rms in soft-symbol units */
    double   dc;                     /* sum / (512 n) (I8: 508), the same units */
    double   flip_rate, sat_rate, neg_rate;      /* over n */
    double   esn0_snv_db;            /* 10 log10(m1^2 / (2 (m2 - m1^2))), m1 = s1 / n, m2 = s2 / n */
    double   esn0_m2m4_db;           /* d = 3 s2^2 - n s4 exactly; S = sqrt(d / 2) / n, N = m2 - S: 10 log10(S / (2 N)) */
    uint32_t flags;                  /* XRIT_MONITOR_NO_SIGNAL, XRIT_MONITOR_NO_NOISE */
    uint32_t reserved;
} xrit_monitor_quality;              /* 64 bytes */

/* block: a multiple of 64 in 64 .. 32768, 0 selects 16384.  No device: XRIT_E_NO_DEVICE, "no CPU path". */
int xrit_monitor_create(xrit_monitor **m, uint32_t block, int symbol_type, int device);
int xrit_monitor_destroy(xrit_monitor *m);
/* the state zero; waits for the handle's last call */
int xrit_monitor_reset(xrit_monitor *m);
/* the blocks a push of n symbols will complete: the host keeps symbols_total mod block itself (moved on only by a push
 * that was enqueued), so no read-back is needed to size d_rows */
size_t xrit_monitor_rows(const xrit_monitor *m, size_t n);
/* device pointers, asynchronous on `stream` (0: the null stream), no host synchronisation, no read-back.  d_symbols is
 * aligned to one symbol; the 16-byte loads cover the aligned core of every piece whatever the pointer.  The head of the
 * call completes the open block, every block completed is written to d_rows in stream order (8-byte aligned; may be
 * null when the call completes none), the tail stays open.  cap_rows below xrit_monitor_rows(m, n): XRIT_E_CAPACITY,
 * nothing enqueued, the state untouched.  n = 0 is a call like any other; n above 2^30: XRIT_E_INVALID.  d_summary
 * (8-byte aligned) may be null.  Calls on one handle share its state: keep them in order. */
int xrit_monitor_push_device(xrit_monitor *m, const void *d_symbols, size_t n, xrit_monitor_block *d_rows, size_t cap_rows,
                             xrit_monitor_summary *d_summary, void *stream);
/* host buffers: one upload, one download.  *n_rows: the rows written; with XRIT_E_CAPACITY the rows that were needed */
int xrit_monitor_push(xrit_monitor *m, const void *symbols, size_t n, xrit_monitor_block *rows, size_t cap_rows, size_t *n_rows);
/* the state after the handle's last call (waits for it) */
int xrit_monitor_get_state(xrit_monitor *m, xrit_monitor_state *out);
/* One record in float64: pure host code, never touches a device.  XRIT_E_INVALID for n = 0, n above 32768 or sums that
 * no n lattice values give. */
int xrit_monitor_derive(const xrit_monitor_block *b, int symbol_type, xrit_monitor_quality *q);

/* ------------------------------------------------------------------------
 * Stage objects -- the SatHelper classes one by one, for stage-level parity
 * and for callers that keep the reference's five-Work() structure.
 * in/out are HOST pointers unless the _device variant is used.
 * ------------------------------------------------------------------------ */
typedef struct xrit_fir     xrit_fir;      /* SatHelper::FirFilter      (demodulator.cpp:446,450) */
typedef struct xrit_agc     xrit_agc;      /* SatHelper::AGC            (:447) */
typedef struct xrit_costas  xrit_costas;   /* SatHelper::CostasLoop     (:448) */
typedef struct xrit_clock   xrit_clock;    /* SatHelper::ClockRecovery  (:449) */
typedef struct xrit_rtl     xrit_rtl;      /* RtlFrontend's byte -> float conversion (RtlFrontend.cpp:102-116) */

/* sample_rate: what RtlFrontend::SetSampleRate received (alpha of the DC tracker, RtlFrontend.cpp:57) */
int  xrit_rtl_create(float sample_rate, int device, xrit_rtl **out);
/* n_complex IQ pairs = 2 n_complex bytes in, 2 n_complex floats out (what the frontend passes to its callback) */
int  xrit_rtl_work(xrit_rtl *r, const uint8_t *data, size_t n_complex, float *out_iq);
void xrit_rtl_destroy(xrit_rtl *r);

int  xrit_fir_create(unsigned decimation, const float *taps, int ntaps, int device, xrit_fir **out);
/* FirFilter::Work(in, out, nOut): consumes nOut*decimation samples */
int  xrit_fir_work(xrit_fir *f, const float *in, float *out, size_t n_out);
/* exact = 1: the dot product summed in the CPU chain's order -- four interleaved float32 partial sums over the time-ordered
 * window, products rounded before they are added (xrit_demod_config.front_exact = 2) */
int  xrit_fir_set_exact(xrit_fir *f, int exact);
void xrit_fir_destroy(xrit_fir *f);

int  xrit_agc_create(float rate, float reference, float gain, float max_gain, int device, xrit_agc **out);
int  xrit_agc_work(xrit_agc *a, const float *in, float *out, size_t n);
/* exact = 1: the float32 recurrence walked literally in warmed-up chains whose joints are checked bit for bit (front_exact = 2) */
int  xrit_agc_set_exact(xrit_agc *a, int exact);
/* the last exact call's counters: [0] joints open after the rounds, [1] 64-sample blocks walked, [2] Picard rounds, [3] blocks at the
 * round limit, [4] lattice segments, [5] scans that fell back to the systolic one, [6..7] unused */
int  xrit_agc_exact_stats(xrit_agc *a, uint32_t *counters8);
float xrit_agc_gain(xrit_agc *a);
void xrit_agc_destroy(xrit_agc *a);

int  xrit_costas_create(float loop_bw, int order, int device, xrit_costas **out);
int  xrit_costas_work(xrit_costas *c, const float *in, float *out, size_t n);
int  xrit_costas_state(xrit_costas *c, float *phase, float *freq);
/* exact = 1: behind the chains' hand-off the output is put on the serial float32 trajectory by exactly walked overlapping
 * ranges (front_exact = 2; csrc/costas_exact.hip).  history: samples of warm-up in front of every range (0 = by plan:
 * none on large calls, where a walker goes on into the next range until the two meet; up to 32768 on small ones) */
int  xrit_costas_set_exact(xrit_costas *c, int exact, int history);
/* totals over the handle's calls: 64-sample blocks walked and Picard rounds spent on them; of the last call: joints that were
 * still open after the rounds enqueued with the call, and the rounds the host added; totals again: segments of the lattice
 * scans and scans that fell back to the systolic one (any pointer may be null) */
int  xrit_costas_exact_stats(xrit_costas *c, uint64_t *blocks, uint64_t *rounds, uint32_t *joints_open, uint32_t *fix_rounds,
                             uint64_t *lattice_segments, uint64_t *lattice_fallbacks);
void xrit_costas_destroy(xrit_costas *c);

/* The sincosf of the exact Costas loop on an array of (host) floats, |x| < 120: the C library's sincosf as the reference's loop
 * calls it (glibc's __sincosf_fma: double-precision reduction and polynomials, fused multiply-adds, one rounding), evaluated
 * operation for operation on the device (csrc/exact_sincos.h; tests hold it against the CPU chain's bit for bit). */
int  xrit_loop_sincosf(const float *x, float *sin_out, float *cos_out, size_t n, int device);

int  xrit_clock_create(float omega, float gain_omega, float mu, float gain_mu, float omega_rel_limit,
                       int device, xrit_clock **out);
/* ClockRecovery::Work(in, out, n) -> symbols through n_out */
int  xrit_clock_work(xrit_clock *c, const float *in, size_t n, float *out, size_t cap, size_t *n_out);
/* serial = 1: one trajectory on a single wave (see xrit_demod_config.clock_serial); 0: time-tiled chains (default) */
int  xrit_clock_set_serial(xrit_clock *c, int serial);
/* exact closure of the tiled evaluation (see xrit_demod_config.clock_exact / clock_exact_window) */
int  xrit_clock_set_exact(xrit_clock *c, int exact, int window);
void xrit_clock_destroy(xrit_clock *c);

/* ------------------------------------------------------------------------
 * Synthetic burst generator -- stands in for the cf32 capture
 * the reference reads through CFileFrontend (CFileFrontend.cpp:34-56).
 * Writes n cf32 samples [start, start+n) into a device buffer.
 * ------------------------------------------------------------------------ */
typedef struct xrit_synth_params {
    double   fs_in, symbol_rate, alpha, amplitude, carrier_hz, phase0, timing_offset, clock_ppm;
    double   esn0_db;     /* < -900: no noise */
    uint64_t seed;
} xrit_synth_params;
void xrit_synth_defaults(xrit_synth_params *p);
int  xrit_synth_generate_device(const xrit_synth_params *p, uint64_t start, size_t n,
                                float *d_out_interleaved, int device, void *stream);

/* ------------------------------------------------------------------------
 * One capture across the GPUs of a node.  The reference runs the
 * chain on one CPU thread (demodulator.cpp:170-175); a burst is cut here in
 * `world` time slices, one per GPU, and three small things cross GPUs -- RCCL
 * ncclSend / ncclRecv over xGMI and one ncclAllGather of two integers per rank:
 * the halo (the last xrit_group_halo_samples() input samples of rank g-1, which
 * rank g demodulates first from a cold start), the last 256 soft symbols of rank
 * g-1 (Costas pi ambiguity, straddling symbol), and (relative polarity, symbol
 * count) of every rank (-> absolute polarity, output offset).  Independent
 * capture segments need none of it: every rank uses xrit_group_chain() as a
 * plain chain handle.
 * ------------------------------------------------------------------------ */
typedef struct xrit_group xrit_group;
#define XRIT_GROUP_ID_BYTES 128
/* One process per GPU: rank 0 makes the id (ncclGetUniqueId), the launcher hands
 * it to every rank (environment, file, MPI, torch.distributed ...), every rank
 * calls xrit_group_create with cfg->device = its GPU (collective call). */
int xrit_group_unique_id(void *id /* [XRIT_GROUP_ID_BYTES] */);
int xrit_group_create(const xrit_demod_config *cfg, int rank, int world, const void *id, xrit_group **out);
/* One process driving `world` GPUs (ncclCommInitAll): out[0..world) are the ranks'
 * handles, to be used from one thread each. */
int xrit_group_create_all(const xrit_demod_config *cfg, const int *devices, int world, xrit_group **out);
/* The same exchange without RCCL: ranks are threads of one process that hand
 * their buffers over through device-to-device copies (hipMemcpyPeer across
 * GPUs).  What a single-GPU box can run: several ranks on one device. */
typedef struct xrit_local_fabric xrit_local_fabric;
int  xrit_local_fabric_create(int world, xrit_local_fabric **out);
void xrit_local_fabric_destroy(xrit_local_fabric *f);
int  xrit_group_create_local(const xrit_demod_config *cfg, int rank, xrit_local_fabric *fabric, xrit_group **out);
void xrit_group_destroy(xrit_group *g);
xrit_demod *xrit_group_chain(xrit_group *g);
int    xrit_group_rank(const xrit_group *g);
int    xrit_group_world(const xrit_group *g);
size_t xrit_group_halo_samples(const xrit_group *g);
/* What this rank did at its slice boundaries so far (see xrit_group_process_slice_device): slices started a second time
 * from the other Costas lock; slices whose clock recovery ran again from the loop state of the rank in front; slices
 * that had met that state bit for bit inside their halo (nothing to run again).  Any pointer may be null. */
void xrit_group_counters(const xrit_group *g, uint64_t *relocks, uint64_t *handovers, uint64_t *joined);
/* Ranks of the RCCL communicator the group exchanges over, as RCCL itself counts them (ncclCommCount); 0 when the
 * ranks are threads of one process (xrit_group_create_local: no communicator). */
int    xrit_group_rccl_ranks(xrit_group *g);
/* Collective: every rank passes ITS slice (n samples, device resident, slices in
 * rank order make up the burst; n >= the halo and a whole number of decimation
 * periods) and receives its symbols in the stream's
 * polarity with their offset in the burst's symbol sequence: rank r's symbols are
 * out[offset .. offset + n_out) of what one chain would emit for the whole burst
 * (a rank whose Costas loop locked pi away from the stream's starts once more
 * from a phase of pi where its front end is the bit-exact one -- it then meets the
 * stream's own trajectory inside the halo, like a rank that fell on the right side
 * at once: symbols that are the single chain's word for word wherever that chain's
 * are the CPU chain's --, and with the fast front end runs its clock recovery once
 * more on the sign-flipped stream, so both locks end at the same floor).  Consecutive calls are consecutive bursts of ONE
 * capture: the last rank keeps the end of its slice and hands it to rank 0 at the
 * start of the next call (the exchanges become a ring), so rank 0 warms up over a
 * halo like every other rank; xrit_group_restart() begins a new capture (as does
 * a failed call).  Every slice must be a whole number of decimation periods.
 * A failure on one rank (capacity, a stage that did not converge in strict mode,
 * HIP) is carried to every rank in the all-gather: every rank returns an error
 * from the same call and nobody is left waiting in an exchange; a rank that
 * cannot even serve its peers (out of device memory) aborts the communicator. */
int xrit_group_process_slice_device(xrit_group *g, const void *d_samples, size_t n_complex, int sample_type,
                                    float *d_soft_out, size_t cap, size_t *n_out, uint64_t *offset_out,
                                    int *polarity_out, void *stream);
/* the same with host buffers (one H2D / D2H round trip per call, like xrit_demod_process) */
int xrit_group_process_slice_host(xrit_group *g, const void *samples, size_t n_complex, int sample_type, float *soft_out,
                                  size_t cap, size_t *n_out, uint64_t *offset_out, int *polarity_out);
/* max over the ranks (timing: the slowest rank's seconds) */
int xrit_group_restart(xrit_group *g);   /* the next slice call is a capture's first (every rank calls it) */
int xrit_group_allreduce_max(xrit_group *g, double *value, void *stream);

/* ------------------------------------------------------------------------
 * Measurement helper ("also measure a device read microbenchmark
 * on the box and report both"): GB/s of a hand-written read-only sweep over a
 * device buffer, `reps` sweeps timed with HIP events on `stream`.  Not part of
 * the reference's interface.
 * ------------------------------------------------------------------------ */
int xrit_device_read_bandwidth(const void *d_buf, size_t bytes, int reps, int device, void *stream, double *gb_per_s);

#ifdef __cplusplus
}
#endif
#endif /* XRITDEMOD_AMD_H_ */
