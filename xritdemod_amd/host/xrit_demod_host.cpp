// xrit_demod_host -- the reference demodulator's plumbing around libxritdemod_amd:
// IQ file source -> demodulation chain on the GPU -> int8 soft symbols -> TCP client
// socket towards a decoder (or a file).  It is the host loop SURVEY.md section 8(b)/(f)
// asks for, so that the unmodified xritDecoder listening on :5000 can attach.
//
// What it mirrors of the reference's demodulator/src:
//   * CFileFrontend.cpp:35-60   blocks of complex samples read from a raw IQ file; with
//                               --paced the blocks are released at the capture's sample
//                               rate like the reference does (default: as fast as possible)
//   * demodulator.cpp:100-168   processSamples(): one chain call per block, state carried
//   * demodulator.cpp:38,       --fifo: the reference's chunking rule instead of fixed --block calls: the source delivers blocks of
//     :108-119, Parameters.h:57 --fifo-block samples (65535: CFileFrontend's BUFFERSIZE) into a FIFO of 1 Mi floats (512 Ki complex
//                               samples); the DSP loop looks at it after every --fifo-lag blocks and, once it holds 64 Ki floats,
//                               takes EVERYTHING it holds as one chunk -- so the chunk length varies, and with it which `length
//                               mod decimation` samples :137 drops.  What does not fit the FIFO is lost ("Input Samples Fifo is
//                               overflowing!").  The reference's chunk sizes depend on thread timing; here they are a function of
//                               (--fifo-block, --fifo-lag), so that a run can be repeated and checked against the oracle.
//   * SymbolManager.cpp:37-52   soft symbol -> int8 (x127, clamp, C-cast truncation), sent
//                               in pieces of at most 16384 bytes (SM_SOCKET_BUFFER_SIZE)
//   * SymbolManager.cpp:23-35   the demodulator is the TCP *client*; it retries the
//                               connection once per second until the decoder listens
//   * SymbolManager.cpp:78-106  --drop: the reference's queue between the DSP thread and the sender thread, with its
//                               loss behaviour: a chunk of symbols is DROPPED when 1 Mi symbols are already queued
//                               ("SymbolManager Buffer is full!!! Dropping samples."), and everything queued is
//                               dropped while no decoder is connected.  The default (no --drop) is lossless: the DSP
//                               loop waits for the socket, which is what a file run at GPU speed wants.
//   * decoder/src/Statistics.h:34  --stats reports the queue's fill as demodulatorFifoUsage (percent of its capacity,
//                               one byte like the decoder's statistics field) with its peak and the drop counts
//   * DiagManager.cpp:24-62,    --diag: the constellation tap -- after every chain call up to 1024 floats of
//     demodulator.cpp:161-163   the complex symbols (I, Q interleaved) are queued; whenever 1024 are queued and
//                               10 ms have passed they go out as int8 (x128, clamp, truncation) in one UDP
//                               datagram from port 9001 to HOST:9000
//   * demodulator.cpp:285-290,  --tune HZ / --acquire: the reference tunes its source with the `frequency` key of the config file and is
//     :461                      retuned by hand; a recorded capture is derotated on the device instead (xrit_acquire_*), by a given
//                               offset or by the one estimated on the capture's first samples
//   * DiagManager / the         --monitor FILE: nobody watches a constellation while a recorded capture runs through; per block of
//     decoder's signal quality  soft symbols the level, two Es/N0 estimates and the flip and saturation rates go to a CSV file
//                               (xrit_monitor_*), the run's median and its low blocks to stderr at exit
// Only the C ABI of include/xritdemod_amd.h is used (no HIP headers): this file and the headers next to it build with plain
// g++.  The pieces: options.h (the command line), source.h (what the samples are read through), sinks.h (where the symbols
// go), stages.h (the decode chain behind the symbols, one struct per stage of the library) and outputs.h (the files it
// leaves, as plain file logic).  Here: main and run_multi_gpu.  Everything that is opened is released by scope, so every
// return releases what was opened so far.
#include <atomic>
#include <chrono>
#include <thread>

#include "options.h"
#include "sinks.h"
#include "source.h"
#include "stages.h"

namespace {

bool sample_format(const std::string &format, int &type, size_t &bytes_per_sample)
{
    if (format == "cf32") { type = XRIT_SAMPLE_FLOATIQ; bytes_per_sample = 8; }
    else if (format == "s16") { type = XRIT_SAMPLE_S16IQ; bytes_per_sample = 4; }
    else if (format == "s8") { type = XRIT_SAMPLE_S8IQ; bytes_per_sample = 2; }
    else if (format == "u8") { type = XRIT_SAMPLE_U8IQ; bytes_per_sample = 2; }      // raw rtl_sdr capture
    else return false;
    return true;
}

Source file_source(FILE *in, size_t bytes_per_sample, const Options &o)
{
    Source s;
    s.reader = [in, bytes_per_sample](void *dst, size_t count) { return std::fread(dst, bytes_per_sample, count, in); };
    s.bytes_per_sample = bytes_per_sample;
    s.paced = o.paced;
    s.sample_rate = o.sample_rate;
    s.fifo = o.fifo;
    s.fifo_block = o.fifo_block;
    s.fifo_lag = o.fifo_lag;
    return s;
}

// --tune / --acquire: the stage in front of the chain; what the estimate reads ahead the source hands out again
bool open_acquire(xrit_acquire **acq, const Options &o, Source &source, int type)
{
    xrit_acquire_params ap{};
    ap.sample_rate = o.sample_rate;
    ap.pre_sum = o.acquire_presum;
    if (xrit_acquire_create(acq, &ap, o.device) != XRIT_OK || (o.tune && xrit_acquire_set_frequency(*acq, o.tune_hz) != XRIT_OK)) return false;
    if (!o.acquire) return true;
    const size_t first = o.fifo ? o.fifo_block : o.block, least = (size_t)65536 * o.acquire_presum;
    size_t want = first;
    while (want < least) want += first;         // whole blocks, as many as hold 65536 * R samples
    const size_t got = source.read_ahead(want);
    xrit_acquire_estimate_record rec{};
    if (xrit_acquire_estimate(*acq, source.ahead.data(), got, type, 1, &rec) != XRIT_OK) return false;
    if (rec.status == XRIT_ACQUIRE_OK)
        std::fprintf(stderr, "acquire: carrier offset %.1f Hz, line ratio %.1f over %u segments\n", rec.hz, rec.ratio, rec.segments);
    else if (rec.status == XRIT_ACQUIRE_WEAK)
        std::fprintf(stderr, "acquire: weak: no carrier line stands out (best %.1f Hz, line ratio %.1f over %u segments); not tuned\n",
                     rec.hz, rec.ratio, rec.segments);
    else
        std::fprintf(stderr, "acquire: too short: %zu samples, %zu are needed; not tuned\n", got, least);
    return true;
}

// --diag: the first symbols of the call, complex (stage 4); only what the tap can take is copied back
void tap(Diag &diag, xrit_demod *chain, size_t nsym)
{
    std::vector<float> all;
    size_t have = 0;
    if (xrit_demod_read_stage(chain, 4, nullptr, 0, &have) == XRIT_OK && have > 0) {
        all.resize(2 * have);
        if (xrit_demod_read_stage(chain, 4, all.data(), have, &have) == XRIT_OK) diag.add(all.data(), nsym);
    }
    diag.pump();
}

// --drop: the sender thread next to the DSP loop; finish() (and the scope's end) tells it the DSP is done and waits for it
struct Sender {
    std::atomic<bool> dsp_done{false};
    std::thread thread;
    void start(Sink &sink, SymbolQueue &queue) { thread = std::thread([&sink, &queue, this] { run_sender(sink, queue, dsp_done); }); }
    void finish()
    {
        dsp_done.store(true);
        if (thread.joinable()) thread.join();
    }
    ~Sender() { finish(); }
};

struct Groups {
    std::vector<xrit_group *> g;
    explicit Groups(int n) : g((size_t)n, nullptr) {}
    Groups(const Groups &) = delete;
    Groups &operator=(const Groups &) = delete;
    ~Groups() { for (xrit_group *p : g) if (p) xrit_group_destroy(p); }
};

}  // namespace

// --gpus N: one process drives N GPUs (ncclCommInitAll).  A block of the capture is cut in N time slices, one per
// GPU; the ranks exchange the halo and the boundary symbols over RCCL (xrit_group_process_slice_device) and the
// symbols are sent on in rank order.  Every block starts from cold chains (a rank's previous slice ended somewhere
// else in the stream), so blocks should be long: the halo is ~1 M input samples per rank at LRIT, decimation 5.
static int run_multi_gpu(const Options &o, int type, size_t bytes_per_sample, const xrit_demod_config &cfg0)
{
    const int W = o.gpus;
    if (xrit_device_count() < W) { std::fprintf(stderr, "--gpus %d: only %d HIP devices\n", W, xrit_device_count()); return 1; }
    std::vector<int> devs((size_t)W);
    for (int i = 0; i < W; ++i) devs[(size_t)i] = i;
    Groups groups(W);
    std::vector<xrit_group *> &grp = groups.g;
    if (xrit_group_create_all(&cfg0, devs.data(), W, grp.data()) != XRIT_OK) { library_error(); return 1; }
    File in;
    if (!in.open(o.input, "input", "rb")) return 1;
    Sink sink;
    sink.sndbuf = o.sndbuf;
    if (!sink.open(o.sink, o.connect_tries)) return 1;
    const size_t halo = xrit_group_halo_samples(grp[0]);
    const size_t per = o.block / (size_t)W / cfg0.decimation * cfg0.decimation;
    if (per < halo + 1024) { std::fprintf(stderr, "--block %zu is too short for %d slices with a halo of %zu samples\n", o.block, W, halo); return 2; }
    std::vector<unsigned char> raw(per * (size_t)W * bytes_per_sample);
    const size_t cap = per + 1024;
    std::vector<std::vector<float>> soft((size_t)W, std::vector<float>(cap));
    std::vector<size_t> count((size_t)W, 0);
    std::vector<uint64_t> offset((size_t)W, 0);
    std::vector<int> rcs((size_t)W, 0);
    std::vector<int8_t> q(cap);
    size_t total_in = 0, total_sym = 0;
    int exit_code = 0;
    const auto t_start = std::chrono::steady_clock::now();
    for (;;) {
        const size_t n = std::fread(raw.data(), bytes_per_sample, per * (size_t)W, in.f);
        if (n < per * (size_t)W) { std::fprintf(stderr, n ? "EOF (last %zu samples do not fill the slices: dropped)\n" : "EOF\n", n); break; }
        std::vector<std::thread> th;
        for (int r = 0; r < W; ++r)
            th.emplace_back([&, r] {
                // the slice goes to the rank's GPU through the chain's host entry point's twin: device buffers are the
                // group's business, so use the simplest route -- a device copy owned by this thread
                rcs[(size_t)r] = xrit_group_process_slice_host(grp[(size_t)r], raw.data() + (size_t)r * per * bytes_per_sample, per,
                                                               type, soft[(size_t)r].data(), cap, &count[(size_t)r],
                                                               &offset[(size_t)r], nullptr);
            });
        for (auto &t : th) t.join();
        for (int r = 0; r < W; ++r)
            if (rcs[(size_t)r] != XRIT_OK) { std::fprintf(stderr, "rank %d: %s\n", r, xrit_last_error()); exit_code = 1; }
        if (exit_code) break;
        for (int r = 0; r < W && !exit_code; ++r) {
            // SymbolManager.cpp:43-46 on the host: the ranks' pieces are already in stream order (offset[r] ascending)
            for (size_t i = 0; i < count[(size_t)r]; ++i) q[i] = quantize_i8(soft[(size_t)r][i]);
            if (!sink.send_all(q.data(), count[(size_t)r])) exit_code = 1;
            total_sym += count[(size_t)r];
        }
        total_in += n;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (o.stats)
        std::fprintf(stderr, "samples in %zu, symbols out %zu, %.3f s (%.2f Msamples/s incl. file and PCIe), %d GPUs, halo %zu samples per boundary\n",
                     total_in, total_sym, secs, secs > 0 ? total_in / secs * 1e-6 : 0.0, W, halo);
    return exit_code;
}

int main(int argc, char **argv)
{
    Options o;
    int type;
    size_t bytes_per_sample;
    if (!parse(argc, argv, o) || !sample_format(o.format, type, bytes_per_sample)) { usage(); return 2; }

    xrit_demod_config cfg;
    if (o.mode == "hrit") xrit_demod_config_hrit(&cfg, (float)o.sample_rate, o.decimation);
    else xrit_demod_config_lrit(&cfg, (float)o.sample_rate, o.decimation);
    cfg.device = o.device;
    cfg.front_exact = o.front_exact;
    if (o.gpus > 1) return run_multi_gpu(o, type, bytes_per_sample, cfg);
    Handle<xrit_demod, xrit_demod_destroy> chain;
    if (xrit_demod_create(&cfg, &chain.p) != XRIT_OK) { library_error(); return 1; }      // e.g. no HIP device: there is no CPU path

    File in;
    if (!in.open(o.input, "input", "rb")) return 1;
    Source source = file_source(in.f, bytes_per_sample, o);
    Handle<xrit_acquire, xrit_acquire_destroy> acq;
    if ((o.tune || o.acquire) && !open_acquire(&acq.p, o, source, type)) { library_error(); return 1; }
    DecodeChain decode;
    if (o.decoding() && !decode.open(o)) { decode.close(); return 1; }
    Monitor monitor;
    if (!o.monitor.empty() && !monitor.open(o.monitor, o.monitor_block, o.device)) { decode.close(); return 1; }
    Sink sink;
    SymbolQueue queue;
    queue.cap = o.queue_symbols;
    sink.sndbuf = o.sndbuf;
    Sender sender;
    if (o.drop) {
        if (o.sink.rfind("tcp://", 0) != 0) { std::fprintf(stderr, "--drop needs a tcp:// sink\n"); return 2; }
        if (!sink.set_tcp(o.sink)) return 2;
        sender.start(sink, queue);
    } else if (!sink.open(o.sink, o.connect_tries)) return 1;

    Diag diag;
    if (!o.diag.empty() && (!diag.open(o.diag) || xrit_demod_keep_stages(chain, 2) != XRIT_OK)) {
        std::fprintf(stderr, "diag: cannot set up %s\n", o.diag.c_str());
        return 1;
    }
    const auto t_start = std::chrono::steady_clock::now();
    source.t_release = t_start;
    const size_t max_chunk = source.max_chunk(o.block), cap = max_chunk + 64;
    std::vector<unsigned char> raw(max_chunk * bytes_per_sample);
    std::vector<float> soft(cap);
    std::vector<int8_t> q(cap);
    std::vector<float> mixed(acq ? 2 * max_chunk : 0);
    size_t total_in = 0, total_sym = 0;
    int exit_code = 0, rc = XRIT_OK;
    for (;;) {
        const size_t n = source.next(raw.data(), o.block);
        if (n == 0) { std::fprintf(stderr, "EOF\n"); break; }
        size_t nsym = 0;
        if (acq) {
            rc = xrit_acquire_mix(acq, raw.data(), n, type, mixed.data());
            if (rc != XRIT_OK) { library_error("mix"); exit_code = 1; break; }
            rc = xrit_demod_process(chain, mixed.data(), n, XRIT_SAMPLE_FLOATIQ, soft.data(), cap, &nsym);
        } else {
            rc = xrit_demod_process(chain, raw.data(), n, type, soft.data(), cap, &nsym);
        }
        if (rc != XRIT_OK) { library_error("process"); exit_code = 1; break; }
        if (monitor.mon && !monitor.add(soft.data(), nsym)) { exit_code = 1; break; }
        if (o.drop) {
            queue.add(soft.data(), nsym);         // SymbolManager::add: never waits, may drop
        } else {
            rc = xrit_quantize_i8(chain, soft.data(), q.data(), nsym);
            if (rc != XRIT_OK) { library_error("quantize"); exit_code = 1; break; }
            if (!sink.send_all(q.data(), nsym)) { exit_code = 1; break; }
            if (decode.active() && !decode.add(q.data(), nsym)) { exit_code = 1; break; }
        }
        if (diag.fd >= 0 && nsym > 0) tap(diag, chain, nsym);
        total_in += n;
        total_sym += nsym;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    const size_t fill_at_eof = o.drop ? queue.size() : 0;
    sender.finish();
    if (o.stats) {
        xrit_demod_stats st;
        if (xrit_demod_get_stats(chain, &st) == XRIT_OK)
            std::fprintf(stderr, "samples in %zu, symbols out %zu, %.3f s (%.2f Msamples/s incl. file and PCIe)\n",
                         total_in, total_sym, secs, secs > 0 ? total_in / secs * 1e-6 : 0.0);
        if (o.fifo) source.report_fifo();
        if (o.drop)
            std::fprintf(stderr, "symbol queue: capacity %zu, peak %zu, demodulatorFifoUsage %u %% at end of input (peak %u %%), "
                                 "sent %zu, dropped while full %zu, dropped while disconnected %zu\n",
                         queue.cap, queue.peak, SymbolQueue::usage(fill_at_eof, queue.cap),
                         SymbolQueue::usage(queue.peak, queue.cap), sink.sent, queue.dropped_full,
                         queue.dropped_disconnected);
    }
    sink.close_all();
    decode.close();
    monitor.report();
    return exit_code;
}
