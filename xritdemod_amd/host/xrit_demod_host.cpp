// xrit_demod_host -- the reference demodulator's plumbing around libxritdemod_amd:
// IQ file source -> demodulation chain on the GPU -> int8 soft symbols -> TCP client
// socket towards a decoder (or a file).  It is the host loop SURVEY.md section 8(b)/(f)
// asks for, so that the unmodified xritDecoder listening on :5000 can attach.
//
// What it mirrors of /root/reference/demodulator/src:
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
// Only the C ABI of include/xritdemod_amd.h is used (no HIP headers): this file builds
// with plain g++.
#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xritdemod_amd.h"

namespace {

struct Options {
    std::string mode = "lrit";
    std::string input;
    std::string format = "cf32";
    std::string sink = "tcp://127.0.0.1:5000";
    std::string diag;              // udp://HOST:PORT, empty = off
    double sample_rate = 2.5e6;
    unsigned decimation = 1;
    size_t block = 1u << 22;       // complex samples per chain call (>= 4 Mi when throughput matters)
    int device = 0;
    int connect_tries = 30;
    bool paced = false;
    bool stats = false;
    bool drop = false;             // SymbolManager's queue and loss behaviour instead of back-pressure
    size_t queue_symbols = 1024 * 1024;   // SM_MAX_SYMBOL_BUFFER (SymbolManager.h:23)
    int sndbuf = 0;                // > 0: SO_SNDBUF of the decoder socket (the kernel's default grows to megabytes)
    int gpus = 1;                  // > 1: every block is cut in that many time slices, one per GPU (xrit_group_*)
    bool fifo = false;             // the reference's FIFO chunking (demodulator.cpp:108-119) instead of fixed --block calls
    size_t fifo_block = 65535;     // complex samples per source callback (CFileFrontend.cpp:12 BUFFERSIZE)
    int fifo_lag = 1;              // source blocks that arrive between two looks of the DSP loop
    int front_exact = 0;           // cfg.front_exact: 1 = the Costas loop's final pass warmed up; 2 = the front end bit for bit a CPU chain's
    std::string decode;            // --decode PATH: the decoder's frame steps on the symbols, VCDUs of good frames to PATH
    std::string channels;          // --channels DIR: the good frames' VCDUs split by VCID, DIR/channel_{vcid}.bin
    std::string decoder_stats;     // --decoder-stats PATH: one Statistics_st (4167 bytes) per valid frame
    std::string packets;           // --packets DIR: the CRC-checked space packets, DIR/vc{vcid}_apid{apid}.bin
    std::string files;             // --files DIR: the LRIT/HRIT files, DIR/vc{vcid}_apid{apid}_{serial}.lrit
    bool files_decompress = false; // --files-decompress: the scan lines of rice-coded image files, ..._{serial}.img
    bool canvas = false;           // --canvas: the segment files' lines joined into full images on the device, DIR/<name>.pgm
    unsigned canvas_slots = 8;     // --canvas-slots N: canvases held at a time
    size_t canvas_mib = 32;        // --canvas-mib M: MiB per canvas (32: a 5424 x 5424 8-bit image, 29 419 776 bytes, fits)
    bool products = false;         // --products: with --canvas, every canvas written also as DIR/<name>.view.pgm and .thumb.pgm (xrit_product_*)
    bool product_flags = false;    // --product-tone or --product-factor was given
    xrit_product_params product{XRIT_TONE_EQUALISE, 0, 10000, 8};      // --product-tone linear|equalise|stretch[:LO:HI], --product-factor F
    int jpeg = 0;                  // --jpeg [Q]: with --products, each .view.pgm and .thumb.pgm also as .jpg of quality Q (xrit_jpeg_*); 0: none
    bool project = false;          // --project: with --canvas, every canvas written also on a latitude / longitude grid, DIR/<name>.geo.pgm (xrit_geo_*)
    bool project_flags = false;    // --project-grid or --project-mode was given
    bool project_grid_given = false;   // --project-grid LON0:LAT0:STEP:COLUMNS:ROWS; otherwise the disc's bounding box at 0.05 degrees
    xrit_geo_grid project_grid{XRIT_GEO_EQUIRECT, 0, 0, 0, 0.0, 0.0, 0.05, 0.05};
    uint32_t project_mode = XRIT_GEO_BILINEAR;     // --project-mode nearest|bilinear
    bool stream_sync = false;      // --stream-sync: the stream frame synchroniser (xrit_framer_*) in front of the frame decoder
    int flywheel = 0;              // --flywheel [N]: the frame lock (xrit_lock_*) in place of framer and decoder, flywheelRecheck = N
    bool tune = false;             // --tune HZ: the input derotated by tune_hz in front of the chain (xrit_acquire_*)
    double tune_hz = 0.0;
    bool acquire = false;          // --acquire: that offset estimated on the first input of at least 65536 * R samples
    unsigned acquire_presum = 1;   // --acquire-presum R: samples summed in front of the estimator (|offset| < sample rate / 4R)
    std::string monitor;           // --monitor FILE: one CSV line per block of soft symbols (xrit_monitor_*), a summary on stderr at exit
    unsigned monitor_block = 16384;    // --monitor-block B: symbols per line, a multiple of 64 in 64 .. 32768
};
constexpr size_t FIFO_COMPLEX = 1024 * 1024 / 2;      // FIFO_SIZE floats (Parameters.h:57)
constexpr size_t FIFO_MIN_COMPLEX = 64 * 1024 / 2;    // "Lets wait for more samples" (demodulator.cpp:113)

void usage()
{
    std::fprintf(stderr,
                 "usage: xrit_demod_host --input FILE [--format cf32|s16|s8|u8] [--mode lrit|hrit]\n"
                 "         [--sample-rate HZ] [--decimation D] [--block SAMPLES] [--device N]\n"
                 "         [--sink tcp://HOST:PORT | file:PATH | null] [--connect-tries N] [--paced] [--stats]\n"
                 "         [--diag udp://HOST:PORT] [--drop [--queue-symbols N]] [--sndbuf BYTES]\n"
                 "         [--gpus N]   (devices 0..N-1: each block of --block samples is cut in N time slices, RCCL edge exchange)\n"
                 "         [--fifo [--fifo-block SAMPLES] [--fifo-lag BLOCKS]]   (the reference's FIFO chunking, demodulator.cpp:108-119)\n"
                 "         [--decode PATH]   (correlate, fix, Viterbi, derandomise, RS(255,223) on the GPU: the 892-byte VCDU of every\n"
                 "                            good frame appended to PATH, counts on stderr at exit; --sink null for a decode-only run)\n"
                 "         [--stream-sync]   (with --decode and the options behind it: frames are found by the stream frame synchroniser,\n"
                 "                            which walks the symbols chunk by chunk from where the last frame ended like the reference's\n"
                 "                            decoder, instead of by correlating fixed 16384-symbol windows; resynchronisations on stderr at exit)\n"
                 "         [--flywheel [N]]   (implies --stream-sync: synchroniser and decoder run as the reference's one loop, the frame lock --\n"
                 "                             after a frame that Reed-Solomon accepts only the first 1024 positions of the next chunk are\n"
                 "                             correlated and position 0 is kept if it is the best of them; every N chunks (1..255, default 4,\n"
                 "                             the reference's flywheelRecheck) the whole chunk is correlated again; a token behind the\n"
                 "                             flag that begins with a digit is taken as N, so a bare --flywheel goes last or before an option)\n"
                 "         [--channels DIR]   (the decoder's ChannelWriter: every good VCDU appended to DIR/channel_{vcid}.bin)\n"
                 "         [--decoder-stats PATH]   (the decoder's Statistics_st, 4167 bytes per valid frame; lost packets on stderr at exit)\n"
                 "         [--packets DIR]   (CCSDS space packets out of the channels' VCDUs: every packet whose CRC-16 matches appended whole,\n"
                 "                            header included, to DIR/vc{vcid}_apid{apid}.bin; counts on stderr at exit)\n"
                 "         [--files DIR]   (LRIT/HRIT files out of the space packets: every file appended to DIR/vc{vcid}_apid{apid}_{serial}.lrit.part,\n"
                 "                          renamed to .lrit at its last packet, deleted when it is aborted (a lost or damaged packet); a file that\n"
                 "                          is open at exit stays .part; counts on stderr at exit)\n"
                 "         [--files-decompress]   (with --files: image files whose headers say Rice compression -- one coded line per packet behind a\n"
                 "                                 header-only first packet -- are also decoded on the GPU to ..._{serial}.img: lines x columns raw\n"
                 "                                 samples, uint8 or little-endian uint16; a line that faults is written as decoded and counted)\n"
                 "         [--canvas [--canvas-slots N] [--canvas-mib M]]   (with --files-decompress: GOES sends an image as several segment files;\n"
                 "                                 their lines are placed into full images on the GPU by the segment identification record\n"
                 "                                 (type 128) and every image that is complete is written to DIR/<annotation text>.pgm (binary PGM,\n"
                 "                                 16-bit big-endian above 8 bits; without annotation vc{vcid}_img{image_id}_{call}.pgm); what is\n"
                 "                                 incomplete at exit becomes ....partial.pgm.  N canvases (1..64, default 8) of M MiB (default 32:\n"
                 "                                 a 5424 x 5424 8-bit image fits) are held at a time)\n"
                 "         [--products [--product-tone linear|equalise|stretch[:LO:HI]] [--product-factor F]]   (with --canvas: every canvas that\n"
                 "                                 is written is also toned to 8 bits on the GPU from its histogram -- equalise (default), linear, or\n"
                 "                                 stretch between the percentiles LO and HI per myriad (default 200:9800), value 0 being \"no data\" --\n"
                 "                                 and written as DIR/<name>.view.pgm, and reduced F times (1..64, default 8; pixels without data\n"
                 "                                 left out of the means) as DIR/<name>.thumb.pgm; only these two are downloaded)\n"
                 "         [--jpeg [Q]]           (with --products: the toned image and the thumbnail are also encoded on the GPU where they lie, as\n"
                 "                                 baseline JPEG of quality Q (1..100, default 90) with a restart marker per row of blocks, and\n"
                 "                                 written as DIR/<name>.view.jpg and DIR/<name>.thumb.jpg; only the files' bytes are downloaded)\n"
                 "         [--project [--project-grid LON0:LAT0:STEP:COLUMNS:ROWS] [--project-mode nearest|bilinear]]   (with --canvas: every canvas\n"
                 "                                 that is written is also resampled on the GPU onto a latitude / longitude grid, from the image\n"
                 "                                 navigation record (type 2) of its segment file at line 0, column 0, and written as\n"
                 "                                 DIR/<name>.geo.pgm: column j is LON0 + j * STEP degrees east, row i LAT0 - i * STEP degrees north\n"
                 "                                 (COLUMNS, ROWS 1..16384; default: the earth's disc around the sub-satellite point at 0.05\n"
                 "                                 degrees); bilinear (default; pixels without data left out of the means) or nearest.  A canvas\n"
                 "                                 without such a record is skipped with a line on stderr.  With --products the projected image\n"
                 "                                 is toned too: DIR/<name>.geo.view.pgm)\n"
                 "         [--tune HZ]   (a carrier offset of HZ is taken out on the GPU in front of the chain; cf32, s16 or s8 input, one GPU)\n"
                 "         [--acquire [--acquire-presum R]]   (the carrier offset is estimated on the first input of at least 65536 * R samples --\n"
                 "                                 further blocks are read ahead if a block is shorter --, printed to stderr with the strength of\n"
                 "                                 its spectral line and held for the run; unambiguous below sample rate / (4 R), R 1..64,\n"
                 "                                 default 1; when no line stands out the run goes on untuned.  With --tune the estimate replaces HZ)\n"
                 "         [--monitor FILE [--monitor-block B]]   (the link monitor on the soft symbols of every call: one CSV line per B symbols --\n"
                 "                                 first,n,level,dc,esn0_m2m4_db,esn0_snv_db,flip_rate,sat_rate,flags -- and at exit one line on\n"
                 "                                 stderr: the median Es/N0, the blocks more than 3 dB under it, the share of symbols the int8\n"
                 "                                 sink saturates.  B a multiple of 64 in 64..32768, default 16384 (a coded frame); one GPU.\n"
                 "                                 No lock flag: an unlocked carrier reads 1.5 .. 2.5 dB, and so can a weak link)\n"
                 "         [--front-exact [-1|1|2]]   (cfg.front_exact; default 0: the bit-exact front end on blocks of less than a million symbols;\n"
                 "                                  -1: the fast one always; 1: the Costas loop's final pass warmed up, ~12 %% slower on big blocks;\n"
                 "                                  2: filters, AGC and Costas loop bit for bit a CPU chain's -- soft symbols within 1e-4 rms of it\n"
                 "                                  on every configuration, ~3 x slower on big blocks)\n");
}

// --product-tone: linear | equalise | stretch | stretch:LO:HI (per myriad, 0 <= LO < HI <= 10000; plain stretch is 200:9800)
bool parse_tone(const char *v, xrit_product_params &p)
{
    const std::string t = v;
    if (t == "linear") { p.tone = XRIT_TONE_LINEAR; return true; }
    if (t == "equalise") { p.tone = XRIT_TONE_EQUALISE; return true; }
    if (t == "stretch") { p.tone = XRIT_TONE_STRETCH; p.p_lo = 200; p.p_hi = 9800; return true; }
    if (t.rfind("stretch:", 0) == 0) {
        char *end = nullptr;
        const char *q = v + 8;
        const long lo = std::strtol(q, &end, 10);
        if (end != q && *end == ':') {
            const char *r = end + 1;
            const long hi = std::strtol(r, &end, 10);
            if (end != r && *end == '\0' && lo >= 0 && lo < hi && hi <= 10000) {
                p.tone = XRIT_TONE_STRETCH;
                p.p_lo = (uint32_t)lo;
                p.p_hi = (uint32_t)hi;
                return true;
            }
        }
    }
    std::fprintf(stderr, "--product-tone %s: linear, equalise, stretch or stretch:LO:HI with 0 <= LO < HI <= 10000\n", v);
    return false;
}

// --project-grid LON0:LAT0:STEP:COLUMNS:ROWS
bool parse_project_grid(const char *v, xrit_geo_grid &g)
{
    double lon0 = 0, lat0 = 0, step = 0;
    long columns = 0, rows = 0;
    int used = 0;
    if (std::sscanf(v, "%lf:%lf:%lf:%ld:%ld%n", &lon0, &lat0, &step, &columns, &rows, &used) == 5 && v[used] == '\0' && step > 0.0 &&
        lon0 >= -360.0 && lon0 <= 360.0 && lat0 >= -90.0 && lat0 <= 90.0 && columns >= 1 && columns <= XRIT_GEO_MAX_DIM && rows >= 1 &&
        rows <= XRIT_GEO_MAX_DIM) {
        g = xrit_geo_grid{XRIT_GEO_EQUIRECT, (uint32_t)columns, (uint32_t)rows, 0, lon0, lat0, step, step};
        return true;
    }
    std::fprintf(stderr, "--project-grid %s: LON0:LAT0:STEP:COLUMNS:ROWS with STEP > 0, COLUMNS and ROWS 1..%d\n", v, XRIT_GEO_MAX_DIM);
    return false;
}

bool parse(int argc, char **argv, Options &o)
{
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", name); return nullptr; }
            return argv[++i];
        };
        const char *v = nullptr;
        if (a == "--input") { if (!(v = need("--input"))) return false; o.input = v; }
        else if (a == "--format") { if (!(v = need("--format"))) return false; o.format = v; }
        else if (a == "--mode") { if (!(v = need("--mode"))) return false; o.mode = v; }
        else if (a == "--sink") { if (!(v = need("--sink"))) return false; o.sink = v; }
        else if (a == "--sample-rate") { if (!(v = need("--sample-rate"))) return false; o.sample_rate = std::atof(v); }
        else if (a == "--decimation") { if (!(v = need("--decimation"))) return false; o.decimation = (unsigned)std::atoi(v); }
        else if (a == "--block") { if (!(v = need("--block"))) return false; o.block = (size_t)std::atoll(v); }
        else if (a == "--device") { if (!(v = need("--device"))) return false; o.device = std::atoi(v); }
        else if (a == "--connect-tries") { if (!(v = need("--connect-tries"))) return false; o.connect_tries = std::atoi(v); }
        else if (a == "--diag") { if (!(v = need("--diag"))) return false; o.diag = v; }
        else if (a == "--queue-symbols") { if (!(v = need("--queue-symbols"))) return false; o.queue_symbols = (size_t)std::atoll(v); }
        else if (a == "--sndbuf") { if (!(v = need("--sndbuf"))) return false; o.sndbuf = std::atoi(v); }
        else if (a == "--gpus") { if (!(v = need("--gpus"))) return false; o.gpus = std::atoi(v); }
        else if (a == "--fifo-block") { if (!(v = need("--fifo-block"))) return false; o.fifo_block = (size_t)std::atoll(v); }
        else if (a == "--fifo-lag") { if (!(v = need("--fifo-lag"))) return false; o.fifo_lag = std::atoi(v); }
        else if (a == "--decode") { if (!(v = need("--decode"))) return false; o.decode = v; }
        else if (a == "--channels") { if (!(v = need("--channels"))) return false; o.channels = v; }
        else if (a == "--decoder-stats") { if (!(v = need("--decoder-stats"))) return false; o.decoder_stats = v; }
        else if (a == "--packets") { if (!(v = need("--packets"))) return false; o.packets = v; }
        else if (a == "--files") { if (!(v = need("--files"))) return false; o.files = v; }
        else if (a == "--files-decompress") o.files_decompress = true;
        else if (a == "--canvas") o.canvas = true;
        else if (a == "--canvas-slots") { if (!(v = need("--canvas-slots"))) return false; o.canvas_slots = (unsigned)std::atoi(v); }
        else if (a == "--canvas-mib") { if (!(v = need("--canvas-mib"))) return false; o.canvas_mib = (size_t)std::atoll(v); }
        else if (a == "--products") o.products = true;
        else if (a == "--product-tone") { if (!(v = need("--product-tone")) || !parse_tone(v, o.product)) return false; o.product_flags = true; }
        else if (a == "--product-factor") {
            if (!(v = need("--product-factor"))) return false;
            char *end = nullptr;
            const long f = std::strtol(v, &end, 10);
            if (*v == '\0' || *end != '\0' || f < 1 || f > XRIT_PRODUCT_MAX_FACTOR) {
                std::fprintf(stderr, "--product-factor %s: 1..%d\n", v, XRIT_PRODUCT_MAX_FACTOR);
                return false;
            }
            o.product.factor = (uint32_t)f;
            o.product_flags = true;
        }
        else if (a == "--jpeg") {
            o.jpeg = 90;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {      // a token that begins with a digit is Q, whole
                char *end = nullptr;
                const long q = std::strtol(argv[++i], &end, 10);
                if (*end != '\0' || q < 1 || q > 100) { std::fprintf(stderr, "--jpeg %s: 1..100\n", argv[i]); return false; }
                o.jpeg = (int)q;
            }
        }
        else if (a == "--project") o.project = true;
        else if (a == "--project-grid") {
            if (!(v = need("--project-grid")) || !parse_project_grid(v, o.project_grid)) return false;
            o.project_flags = o.project_grid_given = true;
        }
        else if (a == "--project-mode") {
            if (!(v = need("--project-mode"))) return false;
            if (std::string(v) == "nearest") o.project_mode = XRIT_GEO_NEAREST;
            else if (std::string(v) == "bilinear") o.project_mode = XRIT_GEO_BILINEAR;
            else { std::fprintf(stderr, "--project-mode %s: nearest or bilinear\n", v); return false; }
            o.project_flags = true;
        }
        else if (a == "--stream-sync") o.stream_sync = true;
        else if (a == "--tune") { if (!(v = need("--tune"))) return false; o.tune = true; o.tune_hz = std::atof(v); }
        else if (a == "--acquire") o.acquire = true;
        else if (a == "--acquire-presum") { if (!(v = need("--acquire-presum"))) return false; o.acquire_presum = (unsigned)std::atoi(v); }
        else if (a == "--monitor") { if (!(v = need("--monitor"))) return false; o.monitor = v; }
        else if (a == "--monitor-block") { if (!(v = need("--monitor-block"))) return false; o.monitor_block = (unsigned)std::atoi(v); }
        else if (a == "--flywheel") {
            o.flywheel = 4;                 // parameters.h:41
            o.stream_sync = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {      // a token that begins with a digit is N, whole
                char *end = nullptr;
                const long r = std::strtol(argv[++i], &end, 10);
                if (*end != '\0' || r < 1 || r > 255) { std::fprintf(stderr, "--flywheel %s: 1..255\n", argv[i]); return false; }
                o.flywheel = (int)r;
            }
        }
        else if (a == "--fifo") o.fifo = true;
        else if (a == "--front-exact") {
            o.front_exact = 1;
            if (i + 1 < argc && (std::string(argv[i + 1]) == "1" || std::string(argv[i + 1]) == "2" || std::string(argv[i + 1]) == "-1")) o.front_exact = atoi(argv[++i]);
        }
        else if (a == "--drop") o.drop = true;
        else if (a == "--paced") o.paced = true;
        else if (a == "--stats") o.stats = true;
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return false; }
    }
    if (o.fifo && (o.fifo_block < 1 || o.fifo_block > FIFO_COMPLEX || o.fifo_lag < 1 || o.gpus > 1)) {
        std::fprintf(stderr, "--fifo: --fifo-block 1..%zu, --fifo-lag >= 1, one GPU\n", FIFO_COMPLEX);
        return false;
    }
    if (!o.decode.empty() && (o.drop || o.gpus > 1)) {
        std::fprintf(stderr, "--decode: one GPU, without --drop\n");
        return false;
    }
    if ((!o.channels.empty() || !o.decoder_stats.empty()) && (o.drop || o.gpus > 1)) {
        std::fprintf(stderr, "--channels / --decoder-stats: one GPU, without --drop\n");
        return false;
    }
    if (!o.packets.empty() && (o.drop || o.gpus > 1)) {
        std::fprintf(stderr, "--packets: one GPU, without --drop\n");
        return false;
    }
    if (!o.files.empty() && (o.drop || o.gpus > 1)) {
        std::fprintf(stderr, "--files: one GPU, without --drop\n");
        return false;
    }
    if (o.stream_sync && o.decode.empty() && o.channels.empty() && o.decoder_stats.empty() && o.packets.empty() && o.files.empty()) {
        std::fprintf(stderr, "--stream-sync needs --decode, --channels, --decoder-stats, --packets or --files\n");
        return false;
    }
    if (o.files_decompress && o.files.empty()) {
        std::fprintf(stderr, "--files-decompress needs --files DIR\n");
        return false;
    }
    if (o.canvas && (!o.files_decompress || o.canvas_slots < 1 || o.canvas_slots > XRIT_CANVAS_MAX_SLOTS || o.canvas_mib < 1 ||
                     o.canvas_mib > 4096)) {
        std::fprintf(stderr, "--canvas needs --files DIR --files-decompress; --canvas-slots 1..%d, --canvas-mib 1..4096\n", XRIT_CANVAS_MAX_SLOTS);
        return false;
    }
    if ((o.products && !o.canvas) || (o.product_flags && !o.products)) {
        std::fprintf(stderr, "--products needs --canvas; --product-tone and --product-factor need --products\n");
        return false;
    }
    if (o.jpeg && !o.products) {
        std::fprintf(stderr, "--jpeg needs --products\n");
        return false;
    }
    if ((o.project && !o.canvas) || (o.project_flags && !o.project)) {
        std::fprintf(stderr, "--project needs --canvas; --project-grid and --project-mode need --project\n");
        return false;
    }
    if ((o.tune || o.acquire) && (o.gpus > 1 || o.format == "u8" || o.acquire_presum < 1 || o.acquire_presum > 64)) {
        std::fprintf(stderr, "--tune / --acquire: one GPU; cf32, s16 or s8 input; --acquire-presum 1..64\n");
        return false;
    }
    if (!o.monitor.empty() && (o.gpus > 1 || o.monitor_block < 64 || o.monitor_block > 32768 || o.monitor_block % 64)) {
        std::fprintf(stderr, "--monitor: one GPU; --monitor-block a multiple of 64 in 64..32768\n");
        return false;
    }
    return !o.input.empty() && o.block > 0 && o.decimation >= 1 && o.gpus >= 1;
}

// ---- --monitor: the link monitor's rows as CSV, and what the run's summary needs ------------------------------------------
struct MonitorLog {
    xrit_monitor *mon = nullptr;
    FILE *csv = nullptr;
    std::vector<xrit_monitor_block> rows;
    std::vector<double> esn0;           // esn0_m2m4_db of every block, for the median
    uint64_t symbols = 0, sat = 0;

    bool open(const std::string &path, unsigned block, int device)
    {
        if (xrit_monitor_create(&mon, block, XRIT_SYMBOL_F32, device) != XRIT_OK) {
            std::fprintf(stderr, "monitor: %s\n", xrit_last_error());
            return false;
        }
        csv = std::fopen(path.c_str(), "w");
        if (!csv) { std::perror("monitor"); return false; }
        std::fprintf(csv, "first,n,level,dc,esn0_m2m4_db,esn0_snv_db,flip_rate,sat_rate,flags\n");
        return true;
    }
    bool add(const float *soft, size_t n)
    {
        rows.resize(xrit_monitor_rows(mon, n) + 1);
        size_t got = 0;
        if (xrit_monitor_push(mon, soft, n, rows.data(), rows.size(), &got) != XRIT_OK) {
            std::fprintf(stderr, "monitor: %s\n", xrit_last_error());
            return false;
        }
        for (size_t i = 0; i < got; ++i) {
            xrit_monitor_quality q;
            if (xrit_monitor_derive(&rows[i], XRIT_SYMBOL_F32, &q) != XRIT_OK) {
                std::fprintf(stderr, "monitor: %s\n", xrit_last_error());
                return false;
            }
            std::fprintf(csv, "%llu,%u,%.6f,%.6f,%.3f,%.3f,%.6f,%.6f,%u\n", (unsigned long long)rows[i].first, rows[i].n, q.level, q.dc,
                         q.esn0_m2m4_db, q.esn0_snv_db, q.flip_rate, q.sat_rate, q.flags);
            esn0.push_back(q.esn0_m2m4_db);
            symbols += rows[i].n;
            sat += rows[i].sat;
        }
        return true;
    }
    // the median over the run (the upper of the two middle blocks), the blocks more than 3 dB under it, the sink's saturation
    void close()
    {
        if (csv) std::fclose(csv);
        if (mon && csv) {
            if (esn0.empty()) {
                std::fprintf(stderr, "monitor: no block completed\n");
            } else {
                std::vector<double> sorted(esn0);
                std::sort(sorted.begin(), sorted.end());
                const double median = sorted[sorted.size() / 2];
                size_t low = 0;
                for (double v : esn0) low += v < median - 3.0;
                std::fprintf(stderr, "monitor: %zu blocks, median Es/N0 %.2f dB, %zu blocks more than 3 dB under it, %.4f %% of the symbols saturate int8\n",
                             esn0.size(), median, low, 100.0 * (double)sat / (double)symbols);
            }
        }
        if (mon) xrit_monitor_destroy(mon);
        mon = nullptr;
        csv = nullptr;
    }
};

// ---- --decode: the decoder's steps per frame (decoder/src/newdecoder.cpp:218-359) on the quantised symbols -------------
// Whole 16384-symbol windows go through the correlator, the frame fix (HRIT: word forced to 0, NRZ-M takes the phase) and
// the frame decoder; the symbols from the first window whose frame is not complete yet wait for the next round.
// --channels / --decoder-stats add the channel demultiplexer behind the decoder (:309-395): ChannelWriter's files and
// the Statistics_st stream, from the correlator's hits as it returned them.  --packets adds the packet assembler behind
// the demultiplexer: the channels' rows go back to the device and come out as CRC-checked space packets.  --files adds
// the file assembler behind that (and, with --files-decompress, the image stage: the lines of rice-coded image files).
struct FrameDecode {
    static constexpr size_t FRAME = 16384, VCDU = 892;
    static constexpr uint32_t MIN_CORRELATION = 46;     // MINCORRELATIONBITS (parameters.h:31)
    FILE *out = nullptr;
    FILE *stats_out = nullptr;
    xrit_decoder *dec = nullptr;
    xrit_framer *fr = nullptr;      // --stream-sync
    xrit_lock *lk = nullptr;        // --flywheel: in place of fr and dec
    std::vector<uint8_t> modes;
    std::vector<uint64_t> starts;
    xrit_framer_counters fr_stats{};
    xrit_demux *dm = nullptr;
    xrit_packets *pk = nullptr;
    std::string channel_dir, packet_dir;
    std::unique_ptr<uint8_t[]> pk_bytes;
    std::unique_ptr<xrit_packet[]> pk_desc;
    size_t pk_bytes_cap = 0, pk_desc_cap = 0;
    std::map<std::pair<int, int>, FILE *> pk_files;
    xrit_packets_summary pk_summary{};
    xrit_files *fa = nullptr;
    std::string file_dir;
    bool decompress = false;
    std::vector<uint8_t> f_bytes, img;
    std::vector<xrit_file_piece> f_pieces;
    std::vector<xrit_file_record> f_recs;
    xrit_files_summary f_summary{};
    xrit_images *im = nullptr;      // --files-decompress
    std::vector<xrit_image_line> im_lines;
    std::vector<xrit_image_file> im_files;
    xrit_images_summary im_summary{};
    size_t rice_lines = 0, rice_faults = 0;
    xrit_canvas *cv = nullptr;      // --canvas (set canvas_slots and canvas_bytes before open())
    unsigned canvas_slots = 0;
    size_t canvas_bytes = 0;
    std::vector<xrit_canvas_file> cv_files;
    std::vector<xrit_canvas_slot> cv_slots;
    std::vector<uint8_t> cv_pixels, cv_row;
    xrit_canvas_summary cv_summary{};
    size_t canvases_written = 0;
    bool products = false;          // --products (set it and product before open())
    xrit_product_params product{};
    xrit_product *pr = nullptr;
    std::vector<uint8_t> pr_tone, pr_small;
    size_t products_written = 0, product_fallbacks = 0;
    int jpeg = 0;                   // --jpeg's quality, 0: none (set it before open())
    xrit_jpeg *jp = nullptr;
    std::vector<uint8_t> jp_file;
    size_t jpegs_written = 0, jpeg_bytes = 0;
    bool project = false;           // --project (set it, project_grid, project_grid_given and project_mode before open())
    bool project_grid_given = false;
    xrit_geo_grid project_grid{};
    uint32_t project_mode = XRIT_GEO_BILINEAR;
    xrit_geo *geo = nullptr;
    struct SlotNav { int state = 0; xrit_geo_nav nav{}; };      // 0: no file at (0, 0) yet; 1: its record parsed; 2: it did not
    std::vector<SlotNav> geo_nav;   // per canvas slot
    bool geo_grid_set = false;
    double geo_grid_lon = 0.0;      // the sub-satellite longitude the tables in effect were made for
    std::vector<uint8_t> geo_out, geo_tone;
    size_t projected = 0, projections_skipped = 0;
    std::vector<xrit_sync_hit> raw_hits;
    std::vector<uint8_t> vcdu, wire;
    std::vector<xrit_frame_stats> records;
    xrit_decoder_stats dm_stats{};
    bool hrit = false;
    int device = 0;
    std::vector<int8_t> pending;
    std::vector<xrit_sync_hit> hits;
    std::vector<int8_t> frames;
    std::vector<uint8_t> valid, cadu, block;
    std::vector<xrit_frame_info> info;
    size_t n_frames = 0, n_ok = 0, n_dropped = 0, rs_corrections = 0, viterbi_errors = 0;

    bool open(const std::string &path, const std::string &channels, const std::string &stats_path, const std::string &packets,
              const std::string &files, bool files_decompress, bool hrit_mode, int dev, bool stream_sync = false,
              int flywheel = 0)
    {
        hrit = hrit_mode;
        device = dev;
        if (flywheel) {
            if (xrit_lock_create(&lk, hrit ? 1 : 0, device) != XRIT_OK || xrit_lock_set_flywheel(lk, (uint32_t)flywheel) != XRIT_OK) {
                std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                return false;
            }
        } else if (xrit_decoder_create(&dec, hrit ? 1 : 0, device) != XRIT_OK) {
            std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
            return false;
        }
        if (stream_sync && !flywheel && xrit_framer_create(&fr, hrit ? 1 : 0, device) != XRIT_OK) {
            std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
            return false;
        }
        if (!path.empty()) {
            out = std::fopen(path.c_str(), "wb");
            if (!out) { std::perror("decode output"); return false; }
        }
        if (channels.empty() && stats_path.empty() && packets.empty() && files.empty()) return true;
        if (xrit_demux_create(&dm, device) != XRIT_OK || xrit_demux_stats(dm, &dm_stats) != XRIT_OK) {
            std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
            return false;
        }
        if (!channels.empty()) {
            if (::mkdir(channels.c_str(), 0755) != 0 && errno != EEXIST) { std::perror("--channels"); return false; }
            channel_dir = channels;
        }
        if (!stats_path.empty()) {
            stats_out = std::fopen(stats_path.c_str(), "wb");
            if (!stats_out) { std::perror("decoder statistics output"); return false; }
        }
        if (!packets.empty() || !files.empty()) {
            if (xrit_packets_create(&pk, device) != XRIT_OK) {
                std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                return false;
            }
        }
        if (!packets.empty()) {
            if (::mkdir(packets.c_str(), 0755) != 0 && errno != EEXIST) { std::perror("--packets"); return false; }
            packet_dir = packets;
        }
        if (!files.empty()) {
            if (xrit_files_create(&fa, device) != XRIT_OK) {
                std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                return false;
            }
            if (::mkdir(files.c_str(), 0755) != 0 && errno != EEXIST) { std::perror("--files"); return false; }
            file_dir = files;
            decompress = files_decompress;
            if (decompress && xrit_images_create(&im, device) != XRIT_OK) {
                std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                return false;
            }
            if (decompress && canvas_slots) {
                if (xrit_canvas_create(&cv, device, canvas_slots, canvas_bytes) != XRIT_OK) {
                    std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                    return false;
                }
                cv_slots.assign(canvas_slots, xrit_canvas_slot{});
                cv_pixels.resize(canvas_bytes);
                if (products && xrit_product_create(&pr, device) != XRIT_OK) {
                    std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                    return false;
                }
                if (products && jpeg && xrit_jpeg_create(&jp, device) != XRIT_OK) {
                    std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                    return false;
                }
                if (project && xrit_geo_create(&geo, device) != XRIT_OK) {
                    std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
                    return false;
                }
                geo_nav.assign(canvas_slots, SlotNav{});
            }
        }
        return true;
    }
    // --stream-sync: the framer keeps the cursor and the unconsumed symbols on the device; its rows are what the fixed windows'
    // correlate + fix give, found chunk by chunk from where the last frame ended
    bool sync_stream(const int8_t *sym, size_t n, size_t &take)
    {
        const size_t cap = xrit_framer_rows(fr, n);
        hits.resize(cap);
        frames.resize(cap * FRAME);
        valid.resize(cap);
        starts.resize(cap);
        const int got = xrit_framer_push(fr, sym, n, frames.data(), valid.data(), hits.data(), starts.data());
        if (got < 0) return fail("frame synchroniser");
        take = (size_t)got;
        raw_hits.assign(hits.begin(), hits.begin() + (std::ptrdiff_t)take);
        return true;
    }
    // --flywheel: the lock's rows are the framer's and the decoder's at once
    bool lock_stream(const int8_t *sym, size_t n, size_t &take)
    {
        const size_t cap = xrit_lock_rows(lk, n);
        hits.resize(cap);
        frames.resize(cap * FRAME);
        valid.resize(cap);
        starts.resize(cap);
        modes.resize(cap);
        cadu.resize(cap * 1024);
        block.resize(cap * 1020);
        info.resize(cap);
        const int got = xrit_lock_push(lk, sym, n, frames.data(), valid.data(), hits.data(), starts.data(), modes.data(), cadu.data(),
                                       block.data(), info.data());
        if (got < 0) return fail("frame lock");
        take = (size_t)got;
        raw_hits.assign(hits.begin(), hits.begin() + (std::ptrdiff_t)take);
        return true;
    }
    bool add(const int8_t *sym, size_t n)
    {
        if (lk) {
            size_t take = 0;
            if (!lock_stream(sym, n, take)) return false;
            return take == 0 || account_frames(take);
        }
        if (fr) {
            size_t take = 0;
            if (!sync_stream(sym, n, take)) return false;
            return take == 0 || decode_frames(take);
        }
        pending.insert(pending.end(), sym, sym + n);
        const size_t nw = pending.size() / FRAME;
        if (nw == 0) return true;
        // newdecoder.cpp:21-24
        const uint64_t words[2] = {hrit ? 0xfc4ef4fd0cc2df89ull : 0xfca2b63db00d9794ull, hrit ? 0x25010b02f33d2076ull : 0x035d49c24ff2686bull};
        hits.resize(nw);
        frames.resize(nw * FRAME);
        valid.resize(nw);
        if (xrit_sync_correlate(pending.data(), nw * FRAME, words, 2, FRAME, hits.data(), device) != XRIT_OK) return fail("correlate");
        size_t take = nw;           // windows decoded this round
        raw_hits.assign(hits.begin(), hits.end());     // the demux takes the phase as the correlator found it
        for (size_t f = 0; f < nw; ++f) {
            if (hrit) hits[f].word = 0;
            if (hits[f].correlation >= MIN_CORRELATION && f * FRAME + hits[f].position + FRAME > pending.size()) { take = f; break; }
        }
        if (take == 0) return true;
        if (xrit_sync_fix_frames(pending.data(), pending.size(), hits.data(), FRAME, MIN_CORRELATION, frames.data(), valid.data(),
                                 device) != XRIT_OK)
            return fail("fix frames");
        if (!decode_frames(take)) return false;
        pending.erase(pending.begin(), pending.begin() + (std::ptrdiff_t)(take * FRAME));
        return true;
    }
    // the frame decoder and the stages behind it on the first `take` rows of frames / valid / raw_hits
    bool decode_frames(size_t take)
    {
        cadu.resize(take * 1024);
        block.resize(take * 1020);
        info.resize(take);
        if (xrit_decoder_decode(dec, frames.data(), valid.data(), take, cadu.data(), block.data(), info.data()) != XRIT_OK)
            return fail("decode");
        return account_frames(take);
    }
    // the counts, the VCDUs of the good frames and the stages behind the decoder on the first `take` rows of cadu / block / info
    bool account_frames(size_t take)
    {
        for (size_t f = 0; f < take; ++f) {
            if (!info[f].valid) continue;
            ++n_frames;
            viterbi_errors += info[f].viterbi_errors;
            if (!info[f].ok) { ++n_dropped; continue; }
            ++n_ok;
            for (int k = 0; k < 4; ++k) rs_corrections += info[f].rs_errors[k] > 0 ? (size_t)info[f].rs_errors[k] : 0;
            if (out && std::fwrite(block.data() + f * 1020, 1, VCDU, out) != VCDU) { std::perror("decode output"); return false; }
        }
        return !dm || demux(take);
    }
    // ChannelWriter::writeChannel per good frame (newdecoder.cpp:356-360) and the statistics record of every valid frame
    bool demux(size_t take)
    {
        uint32_t off[65];
        vcdu.resize(take * VCDU);
        records.resize(take);
        const xrit_decoder_stats start = dm_stats;
        if (xrit_demux_process(dm, raw_hits.data(), cadu.data(), block.data(), info.data(), take, vcdu.data(), off,
                               records.data()) != XRIT_OK || xrit_demux_stats(dm, &dm_stats) != XRIT_OK)
            return fail("demux");
        for (int v = 0; !channel_dir.empty() && v < 64; ++v) {
            if (off[v + 1] == off[v]) continue;
            const std::string name = channel_dir + "/channel_" + std::to_string(v) + ".bin";
            FILE *f = std::fopen(name.c_str(), "ab");
            const size_t bytes = (size_t)(off[v + 1] - off[v]) * VCDU;
            const bool ok = f && std::fwrite(vcdu.data() + (size_t)off[v] * VCDU, 1, bytes, f) == bytes;
            if (f) std::fclose(f);
            if (!ok) { std::perror(name.c_str()); return false; }
        }
        if (stats_out) {
            wire.resize(take * XRIT_STATISTICS_WIRE_BYTES);
            const int n = xrit_demux_expand(&start, records.data(), take, wire.data());
            if (n < 0) return fail("statistics");
            const size_t bytes = (size_t)n * XRIT_STATISTICS_WIRE_BYTES;
            if (std::fwrite(wire.data(), 1, bytes, stats_out) != bytes) { std::perror("decoder statistics output"); return false; }
        }
        return pk ? assemble(off) : true;
    }
    // the space packets of this round's rows; what has begun and not ended waits on the device for the next round
    bool assemble(const uint32_t *off)
    {
        const size_t rows = off[64], need_bytes = XRIT_PACKETS_MAX_BYTES(rows), need_desc = 127 * rows + 64;
        if (need_bytes > pk_bytes_cap) { pk_bytes.reset(new uint8_t[need_bytes]); pk_bytes_cap = need_bytes; }
        if (need_desc > pk_desc_cap) { pk_desc.reset(new xrit_packet[need_desc]); pk_desc_cap = need_desc; }
        uint32_t pkt_off[65];
        if (xrit_packets_process(pk, vcdu.data(), off, pk_bytes.get(), pk_bytes_cap, pk_desc.get(), pk_desc_cap, pkt_off,
                                 &pk_summary) != XRIT_OK)
            return fail("packets");
        for (size_t i = 0; !packet_dir.empty() && i < pk_summary.packets; ++i) {
            const xrit_packet &d = pk_desc[i];
            if (!d.crc_ok) continue;
            const std::pair<int, int> key{d.vcid, d.apid};
            if (pk_files.size() >= 64 && !pk_files.count(key)) close_packet_files();     // (a bound on the open files)
            FILE *&f = pk_files[key];
            const std::string name = packet_dir + "/vc" + std::to_string(d.vcid) + "_apid" + std::to_string(d.apid) + ".bin";
            if (!f) f = std::fopen(name.c_str(), "ab");
            if (!f || std::fwrite(pk_bytes.get() + d.offset, 1, d.length, f) != d.length) { std::perror(name.c_str()); return false; }
        }
        return fa ? assemble_files(pkt_off) : true;
    }
    // the files of this round's packets: every record's bytes appended to its file, which is renamed at its end and
    // deleted when it is aborted; what is open waits (on the device: the key's state; here: the .part file)
    bool assemble_files(const uint32_t *pkt_off)
    {
        const size_t n = pkt_off[64];
        f_bytes.resize(XRIT_FILES_MAX_BYTES(pk_summary.bytes) + 1);
        f_pieces.resize(XRIT_FILES_MAX_PIECES(n) + 1);
        f_recs.resize(XRIT_FILES_MAX_FILES(n) + 1);
        if (xrit_files_process(fa, pk_bytes.get(), pk_summary.bytes, pk_desc.get(), pkt_off, f_bytes.data(), f_bytes.size(), f_pieces.data(),
                               f_pieces.size(), f_recs.data(), f_recs.size(), &f_summary) != XRIT_OK)
            return fail("files");
        if (decompress && !decode_images()) return false;
        if (cv && !place_lines()) return false;
        for (size_t i = 0; i < f_summary.files; ++i) {
            const xrit_file_record &r = f_recs[i];
            const std::string stem = file_dir + "/vc" + std::to_string(r.vcid) + "_apid" + std::to_string(r.apid) + "_" +
                                     std::to_string(r.key_serial);
            const std::string part = stem + ".lrit.part", img_part = stem + ".img.part";
            const bool begins = r.flags & XRIT_FILE_BEGINS;
            if (r.n_pieces) {
                FILE *f = std::fopen(part.c_str(), begins ? "wb" : "ab");
                const bool ok = f && std::fwrite(f_bytes.data() + r.offset, 1, r.length, f) == r.length;
                if (f) std::fclose(f);
                if (!ok) { std::perror(part.c_str()); return false; }
            }
            // the image stage's verdict: a rice-coded image's record (begun in this round, or open since an earlier one)
            const bool rice = decompress && im_files[i].rice;
            if (rice && begins) {
                FILE *f = std::fopen(img_part.c_str(), "wb");
                if (!f) { std::perror(img_part.c_str()); return false; }
                std::fclose(f);
            }
            if (rice && im_files[i].n_lines) {
                const xrit_image_file &g = im_files[i];
                rice_lines += g.n_lines;
                rice_faults += g.faults;
                // (the stage pads every line to a multiple of 4 bytes; the .img holds them back to back)
                FILE *f = std::fopen(img_part.c_str(), "ab");
                bool ok = f != nullptr;
                for (size_t k = 0; ok && k < g.n_lines; ++k) {
                    const xrit_image_line &ln = im_lines[g.first_line + k];
                    ok = std::fwrite(img.data() + ln.offset, 1, ln.length, f) == ln.length;
                }
                if (f) std::fclose(f);
                if (!ok) { std::perror(img_part.c_str()); return false; }
            }
            if (r.flags & XRIT_FILE_ABORTED) {
                std::remove(part.c_str());
                if (rice) std::remove(img_part.c_str());
            } else if (r.flags & XRIT_FILE_ENDS) {
                if (std::rename(part.c_str(), (stem + ".lrit").c_str()) != 0) { std::perror(part.c_str()); return false; }
                if (rice && std::rename(img_part.c_str(), (stem + ".img").c_str()) != 0) { std::perror(img_part.c_str()); return false; }
            }
        }
        return true;
    }
    // --files-decompress: every Rice-coded line of this round's records in one call; which images are open waits on the device
    bool decode_images()
    {
        size_t bound = 0;           // every piece of a record a line of the record's width, padded
        for (size_t i = 0; i < f_summary.files; ++i)
            bound += (size_t)f_recs[i].n_pieces * (((size_t)f_recs[i].columns * (f_recs[i].bits_per_pixel <= 8 ? 1 : 2) + 3) & ~(size_t)3);
        img.resize(bound + 1);
        im_lines.resize(f_summary.pieces + 1);
        im_files.resize(f_summary.files + 1);
        if (xrit_images_process(im, f_bytes.data(), f_summary.bytes, f_pieces.data(), f_summary.pieces, f_recs.data(), f_summary.files,
                                &f_summary, img.data(), bound, im_lines.data(), f_summary.pieces, im_files.data(), &im_summary) != XRIT_OK)
            return fail("images");
        return true;
    }
    // --canvas: this round's lines into their images' canvases; the ones that became complete are read, written and released
    bool place_lines()
    {
        cv_files.resize(f_summary.files + 1);
        if (xrit_canvas_process(cv, f_bytes.data(), f_summary.bytes, f_pieces.data(), f_summary.pieces, f_recs.data(), f_summary.files,
                                &f_summary, img.data(), im_summary.bytes, im_lines.data(), im_summary.lines, im_files.data(), &im_summary,
                                cv_files.data(), cv_slots.data(), &cv_summary) != XRIT_OK)
            return fail("canvas");
        if (geo) note_navigation();
        for (unsigned s = 0; cv_summary.completed && s < canvas_slots; ++s) {
            if (!cv_slots[s].in_use || !cv_slots[s].complete) continue;
            if (!write_canvas(s, false)) return false;
            if (xrit_canvas_release(cv, s) != XRIT_OK) return fail("canvas release");
            cv_slots[s] = xrit_canvas_slot{};
            if (geo) geo_nav[s] = SlotNav{};
        }
        return true;
    }
    // --project: a canvas's navigation is that of its segment file at line 0, column 0 -- the record in that file's first piece
    void note_navigation()
    {
        for (size_t i = 0; i < f_summary.files; ++i) {
            const xrit_file_record &r = f_recs[i];
            const xrit_canvas_file &c = cv_files[i];
            if (!(r.flags & XRIT_FILE_BEGINS) || c.reason != XRIT_CANVAS_PLACED || c.slot < 0 || (unsigned)c.slot >= canvas_slots ||
                c.start_line || c.start_column || !r.n_pieces)
                continue;
            const xrit_file_piece &first = f_pieces[r.first_piece];
            SlotNav &n = geo_nav[(unsigned)c.slot];
            n.state = xrit_geo_parse_navigation(f_bytes.data() + first.offset, first.length, &n.nav) == XRIT_OK ? 1 : 2;
        }
    }
    // one canvas as binary PGM: DIR/<the annotation text reduced to [A-Za-z0-9._-]>.pgm, or vc<vcid>_img<image_id>_<born_call>
    bool write_canvas(unsigned s, bool partial)
    {
        xrit_canvas_slot info{};
        if (xrit_canvas_read(cv, s, cv_pixels.data(), cv_pixels.size(), &info) != XRIT_OK) return fail("canvas read");
        std::string name;
        for (size_t i = 0; i < sizeof info.name && info.name[i]; ++i) {
            const char c = (char)info.name[i];
            name += (std::isalnum((unsigned char)c) || c == '.' || c == '_' || c == '-') ? c : '_';
        }
        if (name.empty())
            name = "vc" + std::to_string(info.vcid) + "_img" + std::to_string(info.image_id) + "_" + std::to_string(info.born_call);
        const std::string path = file_dir + "/" + name + (partial ? ".partial.pgm" : ".pgm");
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) { std::perror(path.c_str()); return false; }
        const size_t width = info.bits <= 8 ? 1 : 2, row_bytes = (size_t)info.max_column * width;
        bool ok = std::fprintf(f, "P5\n%u %u\n%u\n", info.max_column, info.max_row, (1u << info.bits) - 1u) > 0;
        cv_row.resize(row_bytes);
        for (size_t r = 0; ok && r < info.max_row; ++r) {
            const uint8_t *src = cv_pixels.data() + r * info.pitch;
            if (width == 2) {           // the canvas holds little-endian samples, PGM wants the high byte first
                for (size_t i = 0; i < row_bytes; i += 2) { cv_row[i] = src[i + 1]; cv_row[i + 1] = src[i]; }
                src = cv_row.data();
            }
            ok = std::fwrite(src, 1, row_bytes, f) == row_bytes;
        }
        std::fclose(f);
        if (!ok) { std::perror(path.c_str()); return false; }
        ++canvases_written;
        const std::string stem = file_dir + "/" + name + (partial ? ".partial" : "");
        return (!pr || write_products(s, info, stem)) && (!geo || write_projection(s, info, stem));
    }
    bool write_pgm(const std::string &path, const uint8_t *pixels, uint32_t columns, uint32_t rows, uint32_t bits)
    {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) { std::perror(path.c_str()); return false; }
        const size_t width = bits <= 8 ? 1 : 2, row_bytes = (size_t)columns * width;
        bool ok = std::fprintf(f, "P5\n%u %u\n%u\n", columns, rows, (1u << bits) - 1u) > 0;
        cv_row.resize(row_bytes);
        for (size_t r = 0; ok && r < rows; ++r) {
            const uint8_t *src = pixels + r * row_bytes;
            if (width == 2) {           // little-endian samples, PGM wants the high byte first
                for (size_t i = 0; i < row_bytes; i += 2) { cv_row[i] = src[i + 1]; cv_row[i + 1] = src[i]; }
                src = cv_row.data();
            }
            ok = std::fwrite(src, 1, row_bytes, f) == row_bytes;
        }
        std::fclose(f);
        if (!ok) std::perror(path.c_str());
        return ok;
    }
    // --project: the slot's pixels resampled where they lie; the projected image is what is downloaded
    bool write_projection(unsigned s, const xrit_canvas_slot &info, const std::string &stem)
    {
        if (!info.max_column || !info.max_row) return true;
        const SlotNav &n = geo_nav[s];
        if (n.state != 1) {
            std::fprintf(stderr, "project: %s: %s, not projected\n", stem.c_str(),
                         n.state ? "the image navigation record of its file at line 0, column 0 does not parse" : "no segment file at line 0, column 0");
            ++projections_skipped;
            return true;
        }
        if (!geo_grid_set || geo_grid_lon != n.nav.sub_lon_deg) {           // once per geometry
            xrit_geo_grid g = project_grid;
            if (!project_grid_given) {      // the earth's disc as the satellite sees it: 81.3 degrees either way
                g.columns = g.rows = 3253;
                g.lon0_deg = n.nav.sub_lon_deg - 81.3;
                g.lat0_deg = 81.3;
            }
            if (xrit_geo_set_grid(geo, &g, n.nav.sub_lon_deg) != XRIT_OK) return fail("project grid");
            project_grid = g;
            geo_grid_set = true;
            geo_grid_lon = n.nav.sub_lon_deg;
        }
        xrit_product_image image{nullptr, info.max_column, info.max_row, info.pitch, info.bits};
        if (xrit_canvas_pixels_device(cv, s, &image.d_pixels) != XRIT_OK) return fail("canvas pixels");
        const uint32_t columns = project_grid.columns, rows = project_grid.rows, width = info.bits <= 8 ? 1 : 2;
        geo_out.resize((size_t)columns * rows * width);
        xrit_geo_summary summary{};
        if (xrit_geo_project_resident(geo, &n.nav, &image, project_mode, geo_out.data(), columns * width, &summary) != XRIT_OK)
            return fail("project");
        if (!write_pgm(stem + ".geo.pgm", geo_out.data(), columns, rows, info.bits)) return false;
        ++projected;
        if (!pr) return true;
        // --products: the projected image toned like the canvas
        const xrit_product_image flat{geo_out.data(), columns, rows, columns * width, info.bits};
        geo_tone.resize((size_t)columns * rows);
        xrit_product_summary toned{};
        if (xrit_product_process(pr, &flat, &product, nullptr, nullptr, nullptr, geo_tone.data(), nullptr, &toned) != XRIT_OK)
            return fail("products of the projection");
        return write_pgm(stem + ".geo.view.pgm", geo_tone.data(), columns, rows, 8);
    }
    // --products: the slot's pixels toned and reduced where they lie; the two products are what is downloaded
    bool write_products(unsigned s, const xrit_canvas_slot &info, const std::string &stem)
    {
        if (!info.max_column || !info.max_row) return true;
        xrit_product_image image{nullptr, info.max_column, info.max_row, info.pitch, info.bits};
        if (xrit_canvas_pixels_device(cv, s, &image.d_pixels) != XRIT_OK) return fail("canvas pixels");
        const uint32_t f = product.factor, small_columns = (info.max_column + f - 1) / f, small_rows = (info.max_row + f - 1) / f;
        pr_tone.resize((size_t)info.max_column * info.max_row);
        pr_small.resize((size_t)small_columns * small_rows);
        xrit_product_summary summary{};
        if (xrit_product_process_resident(pr, &image, &product, nullptr, nullptr, nullptr, pr_tone.data(), pr_small.data(), &summary) != XRIT_OK)
            return fail("products");
        product_fallbacks += summary.fallback;
        const struct { const char *ext; const std::vector<uint8_t> *bytes; uint32_t columns, rows; } outs[] = {
            {".view.pgm", &pr_tone, summary.tone_columns, summary.tone_rows}, {".thumb.pgm", &pr_small, summary.small_columns, summary.small_rows}};
        for (const auto &o : outs) {
            const std::string path = stem + o.ext;
            FILE *f = std::fopen(path.c_str(), "wb");
            if (!f) { std::perror(path.c_str()); return false; }
            const bool ok = std::fprintf(f, "P5\n%u %u\n255\n", o.columns, o.rows) > 0 &&
                            std::fwrite(o.bytes->data(), 1, o.bytes->size(), f) == o.bytes->size();
            std::fclose(f);
            if (!ok) { std::perror(path.c_str()); return false; }
        }
        ++products_written;
        if (!jp) return true;
        // --jpeg: both encoded where the product call left them on the device
        const uint8_t *d_tone = nullptr, *d_small = nullptr;
        if (xrit_product_outputs_device(pr, &d_tone, &d_small) != XRIT_OK) return fail("product outputs");
        return write_jpeg(stem + ".view.jpg", d_tone, summary.tone_columns, summary.tone_rows) &&
               write_jpeg(stem + ".thumb.jpg", d_small, summary.small_columns, summary.small_rows);
    }
    // one 8-bit image in device memory as a JPEG file, a restart marker per row of blocks; a file longer than the pixels
    // (noise at a high quality) takes a second call with the room the first one asked for
    bool write_jpeg(const std::string &path, const uint8_t *d_pixels, uint32_t columns, uint32_t rows)
    {
        if (!d_pixels || !columns || !rows) return true;
        if (xrit_jpeg_set_quality(jp, (uint32_t)jpeg, (columns + 7) / 8) != XRIT_OK) return fail("jpeg");
        const xrit_product_image image{d_pixels, columns, rows, columns, 8};
        xrit_jpeg_result result{};
        jp_file.resize((size_t)columns * rows + 4096);
        int rc = xrit_jpeg_encode_resident(jp, &image, 1, jp_file.data(), jp_file.size(), &result);
        if (rc == XRIT_E_CAPACITY) {
            jp_file.resize((size_t)result.size);
            rc = xrit_jpeg_encode_resident(jp, &image, 1, jp_file.data(), jp_file.size(), &result);
        }
        if (rc != XRIT_OK) return fail("jpeg");
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) { std::perror(path.c_str()); return false; }
        const bool ok = std::fwrite(jp_file.data(), 1, (size_t)result.size, f) == (size_t)result.size;
        std::fclose(f);
        if (!ok) { std::perror(path.c_str()); return false; }
        ++jpegs_written;
        jpeg_bytes += (size_t)result.size;
        return true;
    }
    void close_packet_files()
    {
        for (auto &kv : pk_files)
            if (kv.second) std::fclose(kv.second);
        pk_files.clear();
    }
    bool fail(const char *what)
    {
        std::fprintf(stderr, "decode: %s: %s\n", what, xrit_last_error());
        return false;
    }
    void close()
    {
        if (dec || lk)
            std::fprintf(stderr, "decode: %zu frames, %zu ok, %zu dropped, %zu RS corrections, mean Viterbi errors %.2f\n", n_frames,
                         n_ok, n_dropped, rs_corrections, n_frames ? (double)viterbi_errors / (double)n_frames : 0.0);
        if (dec) {
            xrit_decoder_destroy(dec);
            dec = nullptr;
        }
        if (lk) {
            xrit_lock_counters c{};
            if (xrit_lock_stats(lk, &c) == XRIT_OK) {
                std::fprintf(stderr, "sync: %llu symbols, %llu frames, %llu chunks dropped, %llu resynchronisations, %llu symbols left\n",
                             (unsigned long long)c.framer.symbols, (unsigned long long)c.framer.frames,
                             (unsigned long long)c.framer.dropped_chunks, (unsigned long long)c.framer.resyncs,
                             (unsigned long long)c.framer.carry);
                std::fprintf(stderr, "lock: %llu chunks kept at position 0 of the short range, %llu missed there, %llu rechecks, "
                                     "%llu chunks that hung on the frame before, %llu rounds in %llu calls\n",
                             (unsigned long long)c.short_kept, (unsigned long long)c.short_missed, (unsigned long long)c.rechecks,
                             (unsigned long long)c.sensitive_chunks, (unsigned long long)c.rounds, (unsigned long long)c.framer.calls);
            }
            xrit_lock_destroy(lk);
            lk = nullptr;
        }
        if (fr) {
            if (xrit_framer_stats(fr, &fr_stats) == XRIT_OK)
                std::fprintf(stderr, "sync: %llu symbols, %llu frames, %llu chunks dropped, %llu resynchronisations, %llu symbols left\n",
                             (unsigned long long)fr_stats.symbols, (unsigned long long)fr_stats.frames,
                             (unsigned long long)fr_stats.dropped_chunks, (unsigned long long)fr_stats.resyncs,
                             (unsigned long long)fr_stats.carry);
            xrit_framer_destroy(fr);
            fr = nullptr;
        }
        if (dm) {
            std::fprintf(stderr, "demux: lost packets %lld (", (long long)dm_stats.lost_packets);
            const char *sep = "";
            for (int v = 0; v < 64; ++v) {
                if (dm_stats.received[v] < 0) continue;
                std::fprintf(stderr, "%svcid %d: %lld of %lld", sep, v, (long long)dm_stats.lost[v], (long long)dm_stats.received[v]);
                sep = ", ";
            }
            std::fprintf(stderr, ")\n");
            xrit_demux_destroy(dm);
            dm = nullptr;
        }
        if (fa) {
            std::fprintf(stderr, "files: %llu begun, %llu completed, %llu aborted, %llu pieces, %llu bad packets, %llu gaps, %llu orphans\n",
                         (unsigned long long)f_summary.files_begun, (unsigned long long)f_summary.files_completed,
                         (unsigned long long)f_summary.files_aborted, (unsigned long long)f_summary.total_pieces,
                         (unsigned long long)f_summary.bad_packets, (unsigned long long)f_summary.seq_gaps,
                         (unsigned long long)f_summary.orphans);
            if (decompress) std::fprintf(stderr, "rice: %zu lines decoded, %zu faulted\n", rice_lines, rice_faults);
            if (cv) {
                size_t partial = 0;
                for (unsigned s = 0; s < canvas_slots; ++s)
                    if (cv_slots[s].in_use && write_canvas(s, true)) ++partial;
                std::fprintf(stderr, "canvas: %llu images begun, %zu written (%zu of them partial), %llu lines placed, %llu clipped, "
                                     "%llu segment files refused\n",
                             (unsigned long long)cv_summary.canvases_begun, canvases_written, partial,
                             (unsigned long long)cv_summary.lines_placed, (unsigned long long)cv_summary.lines_clipped,
                             (unsigned long long)(cv_summary.bad_segment + cv_summary.too_large + cv_summary.duplicate + cv_summary.overlap +
                                                  cv_summary.no_slot + cv_summary.no_placement));
                if (pr) {
                    std::fprintf(stderr, "products: %zu canvases toned and reduced %u times, %zu of them by the linear fallback\n", products_written,
                                 product.factor, product_fallbacks);
                    xrit_product_destroy(pr);
                    pr = nullptr;
                }
                if (jp) {
                    std::fprintf(stderr, "jpeg: %zu files of quality %d, %zu bytes\n", jpegs_written, jpeg, jpeg_bytes);
                    xrit_jpeg_destroy(jp);
                    jp = nullptr;
                }
                if (geo) {
                    std::fprintf(stderr, "project: %zu canvases projected onto %u x %u (%s), %zu skipped\n", projected, project_grid.columns,
                                 project_grid.rows, project_mode == XRIT_GEO_NEAREST ? "nearest" : "bilinear", projections_skipped);
                    xrit_geo_destroy(geo);
                    geo = nullptr;
                }
                xrit_canvas_destroy(cv);
                cv = nullptr;
            }
            xrit_files_destroy(fa);
            fa = nullptr;
            if (im) xrit_images_destroy(im);
            im = nullptr;
        }
        if (pk) {
            std::fprintf(stderr, "packets: %llu emitted, %llu CRC failures, %llu discarded, %llu fill\n",
                         (unsigned long long)pk_summary.total_packets, (unsigned long long)pk_summary.crc_failures,
                         (unsigned long long)pk_summary.discarded, (unsigned long long)pk_summary.fill_packets);
            close_packet_files();
            xrit_packets_destroy(pk);
            pk = nullptr;
        }
        if (out) std::fclose(out);
        out = nullptr;
        if (stats_out) std::fclose(stats_out);
        stats_out = nullptr;
    }
};

// ---- sink ------------------------------------------------------------------------------------------------
struct Sink {
    enum Kind { NONE, TCP, FILE_ } kind = NONE;
    int fd = -1;
    FILE *f = nullptr;
    std::string host;
    int port = 0;
    int tries = 30;
    int sndbuf = 0;
    size_t sent = 0;

    bool open(const std::string &spec, int connect_tries)
    {
        tries = connect_tries;
        if (spec == "null") { kind = NONE; return true; }
        if (spec.rfind("file:", 0) == 0) {
            kind = FILE_;
            f = std::fopen(spec.c_str() + 5, "wb");
            if (!f) { std::perror("sink file"); return false; }
            return true;
        }
        if (spec.rfind("tcp://", 0) == 0) {
            kind = TCP;
            std::string hp = spec.substr(6);
            size_t c = hp.rfind(':');
            if (c == std::string::npos) { std::fprintf(stderr, "sink: tcp://HOST:PORT expected\n"); return false; }
            host = hp.substr(0, c);
            port = std::atoi(hp.c_str() + c + 1);
            return connect_retry();
        }
        std::fprintf(stderr, "sink: unknown spec %s\n", spec.c_str());
        return false;
    }
    bool connect_once()
    {
        addrinfo hints{}, *res = nullptr;
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_STREAM;
        if (getaddrinfo(host.c_str(), std::to_string(port).c_str(), &hints, &res) != 0 || !res) return false;
        fd = ::socket(res->ai_family, res->ai_socktype, res->ai_protocol);
        if (fd >= 0 && sndbuf > 0) (void)setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &sndbuf, sizeof sndbuf);
        bool ok = fd >= 0 && ::connect(fd, res->ai_addr, res->ai_addrlen) == 0;
        freeaddrinfo(res);
        if (!ok) {
            if (fd >= 0) ::close(fd);
            fd = -1;
            return false;
        }
        int one = 1;
        (void)setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        return true;
    }
    // SymbolManager.cpp:23-35: try, sleep one second, try again
    bool connect_retry()
    {
        for (int t = 0; t < tries; ++t) {
            std::fprintf(stderr, "Trying to connect to decoder at %s:%d\n", host.c_str(), port);
            if (connect_once()) return true;
            std::this_thread::sleep_for(std::chrono::seconds(1));
        }
        std::fprintf(stderr, "sink: no decoder at %s:%d\n", host.c_str(), port);
        return false;
    }
    bool send_all(const int8_t *p, size_t n)
    {
        sent += n;
        if (kind == NONE) return true;
        if (kind == FILE_) return std::fwrite(p, 1, n, f) == n;
        // pieces of at most SM_SOCKET_BUFFER_SIZE bytes, like SymbolManager::process
        while (n > 0) {
            size_t piece = n > 16384 ? 16384 : n;
            ssize_t w = ::send(fd, p, piece, MSG_NOSIGNAL);
            if (w <= 0) {
                std::fprintf(stderr, "Disconnected from decoder.\n");
                ::close(fd);
                fd = -1;
                if (!connect_retry()) return false;
                continue;
            }
            p += w;
            n -= (size_t)w;
        }
        return true;
    }
    void close_all()
    {
        if (fd >= 0) ::close(fd);
        if (f) std::fclose(f);
        fd = -1;
        f = nullptr;
    }
};

// ---- SymbolManager's queue (--drop) ---------------------------------------------------------------------------
// SymbolManager::add / ::process (SymbolManager.cpp:37-52,78-106): the DSP thread queues soft symbols, the sender
// thread takes at most 16384 of them at a time, quantises (x127, clamp, C cast) and sends.  Two ways to lose
// symbols, both kept: add() drops its whole chunk when the queue already holds `cap` symbols, process() empties
// the queue while no decoder is connected.
struct SymbolQueue {
    std::deque<float> q;
    std::mutex m;
    size_t cap = 1024 * 1024;
    size_t dropped_full = 0, dropped_disconnected = 0, peak = 0;

    void add(const float *sym, size_t n)
    {
        std::lock_guard<std::mutex> g(m);
        if (q.size() >= cap) {
            std::fprintf(stderr, "SymbolManager Buffer is full!!! Dropping samples.\n");
            dropped_full += n;
            return;
        }
        q.insert(q.end(), sym, sym + n);
        if (q.size() > peak) peak = q.size();
    }
    size_t take(int8_t *out, size_t max)
    {
        std::lock_guard<std::mutex> g(m);
        const size_t n = q.size() < max ? q.size() : max;
        for (size_t i = 0; i < n; ++i) {
            float f = q.front() * 127;
            f = f > 127 ? 127 : f;
            f = f < -128 ? -128 : f;
            out[i] = (int8_t)(char)f;
            q.pop_front();
        }
        return n;
    }
    void clear_disconnected()
    {
        std::lock_guard<std::mutex> g(m);
        dropped_disconnected += q.size();
        q.clear();
    }
    size_t size()
    {
        std::lock_guard<std::mutex> g(m);
        return q.size();
    }
    // decoder/src/Statistics.h:34: one byte, percent of the capacity (a chunk may overshoot the capacity: clamped)
    static unsigned usage(size_t fill, size_t cap)
    {
        const size_t pc = cap ? fill * 100 / cap : 0;
        return (unsigned)(pc > 255 ? 255 : pc);
    }
};

// ---- constellation tap (DiagManager) -----------------------------------------------------------------------
struct Diag {
    int fd = -1;
    sockaddr_in to{};
    std::deque<float> q;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now() - std::chrono::seconds(1);
    static constexpr size_t CAP = 1u << 16;            // the reference's buffer simply stops taking samples when full

    bool open(const std::string &spec)
    {
        if (spec.rfind("udp://", 0) != 0) { std::fprintf(stderr, "diag: udp://HOST:PORT expected\n"); return false; }
        std::string hp = spec.substr(6);
        size_t c = hp.rfind(':');
        if (c == std::string::npos) return false;
        addrinfo hints{}, *res = nullptr;
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_DGRAM;
        if (getaddrinfo(hp.substr(0, c).c_str(), hp.c_str() + c + 1, &hints, &res) != 0 || !res) return false;
        std::memcpy(&to, res->ai_addr, sizeof to);
        freeaddrinfo(res);
        fd = ::socket(AF_INET, SOCK_DGRAM, 0);
        if (fd < 0) return false;
        sockaddr_in from{};
        from.sin_family = AF_INET;
        from.sin_addr.s_addr = htonl(INADDR_ANY);
        from.sin_port = htons(9001);                   // DiagManager.cpp:30; not fatal if somebody else holds it
        (void)::bind(fd, reinterpret_cast<sockaddr *>(&from), sizeof from);
        return true;
    }
    // demodulator.cpp:161-163: (float *)symbols, min(symbols, 1024) FLOATS
    void add(const float *iq, size_t nsym)
    {
        size_t nf = nsym < 1024 ? nsym : 1024;
        if (q.size() + nf > CAP) return;
        q.insert(q.end(), iq, iq + nf);
    }
    void pump()
    {
        const auto now = std::chrono::steady_clock::now();
        if (q.size() < 1024 || now - last < std::chrono::milliseconds(10)) return;
        char data[1024];
        for (int i = 0; i < 1024; ++i) {
            float v = q.front() * 128.f;
            q.pop_front();
            v = v > 127 ? 127 : v;
            v = v < -128 ? -128 : v;
            data[i] = static_cast<char>(v);
        }
        (void)::sendto(fd, data, sizeof data, 0, reinterpret_cast<const sockaddr *>(&to), sizeof to);
        last = now;
    }
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
    std::vector<xrit_group *> grp((size_t)W, nullptr);
    if (xrit_group_create_all(&cfg0, devs.data(), W, grp.data()) != XRIT_OK) {
        std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
        return 1;
    }
    FILE *in = std::fopen(o.input.c_str(), "rb");
    if (!in) { std::perror("input"); return 1; }
    Sink sink;
    sink.sndbuf = o.sndbuf;
    if (!sink.open(o.sink, o.connect_tries)) { std::fclose(in); return 1; }
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
        const size_t n = std::fread(raw.data(), bytes_per_sample, per * (size_t)W, in);
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
            for (size_t i = 0; i < count[(size_t)r]; ++i) {
                float f = soft[(size_t)r][i] * 127;
                f = f > 127 ? 127 : f;
                f = f < -128 ? -128 : f;
                q[i] = (int8_t)(char)f;
            }
            if (!sink.send_all(q.data(), count[(size_t)r])) exit_code = 1;
            total_sym += count[(size_t)r];
        }
        total_in += n;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (o.stats)
        std::fprintf(stderr, "samples in %zu, symbols out %zu, %.3f s (%.2f Msamples/s incl. file and PCIe), %d GPUs, halo %zu samples per boundary\n",
                     total_in, total_sym, secs, secs > 0 ? total_in / secs * 1e-6 : 0.0, W, halo);
    sink.close_all();
    std::fclose(in);
    for (auto g : grp) xrit_group_destroy(g);
    return exit_code;
}

int main(int argc, char **argv)
{
    Options o;
    if (!parse(argc, argv, o)) { usage(); return 2; }
    int type;
    size_t bytes_per_sample;
    if (o.format == "cf32") { type = XRIT_SAMPLE_FLOATIQ; bytes_per_sample = 8; }
    else if (o.format == "s16") { type = XRIT_SAMPLE_S16IQ; bytes_per_sample = 4; }
    else if (o.format == "s8") { type = XRIT_SAMPLE_S8IQ; bytes_per_sample = 2; }
    else if (o.format == "u8") { type = XRIT_SAMPLE_U8IQ; bytes_per_sample = 2; }      // raw rtl_sdr capture
    else { usage(); return 2; }

    xrit_demod_config cfg;
    if (o.mode == "hrit") xrit_demod_config_hrit(&cfg, (float)o.sample_rate, o.decimation);
    else xrit_demod_config_lrit(&cfg, (float)o.sample_rate, o.decimation);
    int rc = XRIT_OK;
    cfg.device = o.device;
    cfg.front_exact = o.front_exact;
    if (o.gpus > 1) return run_multi_gpu(o, type, bytes_per_sample, cfg);
    xrit_demod *chain = nullptr;
    if (xrit_demod_create(&cfg, &chain) != XRIT_OK) {
        // e.g. no HIP device: there is no CPU path
        std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
        return 1;
    }

    FILE *in = std::fopen(o.input.c_str(), "rb");
    if (!in) { std::perror("input"); xrit_demod_destroy(chain); return 1; }
    // --tune / --acquire: the stage in front of the chain; what the estimate read ahead is handed out again before the file goes on
    xrit_acquire *acq = nullptr;
    std::vector<unsigned char> ahead;
    size_t ahead_pos = 0;
    auto read_samples = [&](void *dst, size_t count) -> size_t {
        if (ahead_pos >= ahead.size()) return std::fread(dst, bytes_per_sample, count, in);
        size_t got = (ahead.size() - ahead_pos) / bytes_per_sample;
        got = got < count ? got : count;
        std::memcpy(dst, ahead.data() + ahead_pos, got * bytes_per_sample);
        ahead_pos += got * bytes_per_sample;
        if (got < count) got += std::fread(static_cast<unsigned char *>(dst) + got * bytes_per_sample, bytes_per_sample, count - got, in);
        return got;
    };
    if (o.tune || o.acquire) {
        xrit_acquire_params ap{};
        ap.sample_rate = o.sample_rate;
        ap.pre_sum = o.acquire_presum;
        bool ok = xrit_acquire_create(&acq, &ap, o.device) == XRIT_OK && (!o.tune || xrit_acquire_set_frequency(acq, o.tune_hz) == XRIT_OK);
        if (ok && o.acquire) {
            const size_t first = o.fifo ? o.fifo_block : o.block, least = (size_t)65536 * o.acquire_presum;
            size_t want = first;
            while (want < least) want += first;         // whole blocks, as many as hold 65536 * R samples
            ahead.resize(want * bytes_per_sample);
            ahead.resize(std::fread(ahead.data(), bytes_per_sample, want, in) * bytes_per_sample);
            xrit_acquire_estimate_record rec{};
            ok = xrit_acquire_estimate(acq, ahead.data(), ahead.size() / bytes_per_sample, type, 1, &rec) == XRIT_OK;
            if (ok && rec.status == XRIT_ACQUIRE_OK)
                std::fprintf(stderr, "acquire: carrier offset %.1f Hz, line ratio %.1f over %u segments\n", rec.hz, rec.ratio, rec.segments);
            else if (ok && rec.status == XRIT_ACQUIRE_WEAK)
                std::fprintf(stderr, "acquire: weak: no carrier line stands out (best %.1f Hz, line ratio %.1f over %u segments); not tuned\n",
                             rec.hz, rec.ratio, rec.segments);
            else if (ok)
                std::fprintf(stderr, "acquire: too short: %zu samples, %zu are needed; not tuned\n", ahead.size() / bytes_per_sample, least);
        }
        if (!ok) {
            std::fprintf(stderr, "xritdemod_amd: %s\n", xrit_last_error());
            if (acq) xrit_acquire_destroy(acq);
            std::fclose(in); xrit_demod_destroy(chain);
            return 1;
        }
    }
    FrameDecode decode;
    decode.canvas_slots = o.canvas ? o.canvas_slots : 0;
    decode.canvas_bytes = o.canvas_mib << 20;
    decode.products = o.products;
    decode.product = o.product;
    decode.jpeg = o.jpeg;
    decode.project = o.project;
    decode.project_grid = o.project_grid;
    decode.project_grid_given = o.project_grid_given;
    decode.project_mode = o.project_mode;
    if ((!o.decode.empty() || !o.channels.empty() || !o.decoder_stats.empty() || !o.packets.empty() || !o.files.empty()) &&
        !decode.open(o.decode, o.channels, o.decoder_stats, o.packets, o.files, o.files_decompress, o.mode == "hrit", o.device, o.stream_sync, o.flywheel)) {
        decode.close(); std::fclose(in); xrit_demod_destroy(chain);
        return 1;
    }
    MonitorLog monitor;
    if (!o.monitor.empty() && !monitor.open(o.monitor, o.monitor_block, o.device)) {
        monitor.close(); decode.close(); std::fclose(in); xrit_demod_destroy(chain);
        return 1;
    }
    Sink sink;
    SymbolQueue queue;
    queue.cap = o.queue_symbols;
    sink.sndbuf = o.sndbuf;
    std::atomic<bool> dsp_done{false};
    std::thread sender;
    if (o.drop) {
        // the reference's symbolThread / process() loop: connect attempts happen HERE, next to the DSP, not before it
        if (o.sink.rfind("tcp://", 0) != 0) { std::fprintf(stderr, "--drop needs a tcp:// sink\n"); std::fclose(in); xrit_demod_destroy(chain); return 2; }
        const std::string hp = o.sink.substr(6);
        const size_t c = hp.rfind(':');
        if (c == std::string::npos) { std::fprintf(stderr, "sink: tcp://HOST:PORT expected\n"); std::fclose(in); xrit_demod_destroy(chain); return 2; }
        sink.kind = Sink::TCP;
        sink.host = hp.substr(0, c);
        sink.port = std::atoi(hp.c_str() + c + 1);
        sender = std::thread([&] {
            std::vector<int8_t> buf(16384);
            bool connected = false;
            int failed = 0;
            for (;;) {
                if (!connected) {
                    std::fprintf(stderr, "Trying to connect to decoder at %s:%d\n", sink.host.c_str(), sink.port);
                    connected = sink.connect_once();
                    if (!connected) {
                        queue.clear_disconnected();          // SymbolManager.cpp:78-83
                        if (dsp_done.load() && ++failed >= 2) return;
                        std::this_thread::sleep_for(std::chrono::seconds(1));
                        continue;
                    }
                }
                const size_t n = queue.take(buf.data(), buf.size());
                if (n == 0) {
                    if (dsp_done.load()) return;
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                    continue;
                }
                size_t off = 0;
                while (off < n) {
                    const ssize_t w = ::send(sink.fd, buf.data() + off, n - off, MSG_NOSIGNAL);
                    if (w <= 0) {
                        std::fprintf(stderr, "Disconnected from decoder.\n");
                        ::close(sink.fd);
                        sink.fd = -1;
                        connected = false;
                        break;                                 // the rest of this piece is lost, like the reference's
                    }
                    off += (size_t)w;
                }
                sink.sent += off;
            }
        });
    } else if (!sink.open(o.sink, o.connect_tries)) { std::fclose(in); xrit_demod_destroy(chain); return 1; }

    Diag diag;
    std::vector<float> diag_iq;
    if (!o.diag.empty()) {
        if (!diag.open(o.diag) || xrit_demod_keep_stages(chain, 2) != XRIT_OK) {
            std::fprintf(stderr, "diag: cannot set up %s\n", o.diag.c_str());
            sink.close_all(); std::fclose(in); xrit_demod_destroy(chain);
            return 1;
        }
        diag_iq.resize(2 * 1024);
    }
    const auto t_start = std::chrono::steady_clock::now();
    auto t_release = t_start;
    const size_t max_chunk = o.fifo ? FIFO_COMPLEX : o.block;
    std::vector<unsigned char> raw(max_chunk * bytes_per_sample);
    const size_t cap = max_chunk + 64;
    // --fifo: samplesFifo (demodulator.cpp:38) between the source's callbacks and the DSP loop
    size_t fifo_fill = 0, fifo_overflowed = 0, fifo_calls = 0, fifo_min = ~(size_t)0, fifo_max = 0;
    bool fifo_eof = false;
    std::vector<unsigned char> blockbuf(o.fifo ? o.fifo_block * bytes_per_sample : 0);
    auto fifo_chunk = [&]() -> size_t {
        // the source runs until the DSP loop looks again AND finds at least 64 Ki floats (:108-116)
        for (;;) {
            for (int b = 0; b < o.fifo_lag && !fifo_eof; ++b) {
                const size_t got = read_samples(blockbuf.data(), o.fifo_block);
                if (got == 0) { fifo_eof = true; break; }
                if (o.paced) {        // CFileFrontend.cpp:36-47: one callback per block period
                    std::this_thread::sleep_until(t_release);
                    t_release += std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                        std::chrono::duration<double>((double)got / o.sample_rate));
                }
                size_t take = got;
                if (fifo_fill + take > FIFO_COMPLEX) {
                    if (!fifo_overflowed) std::fprintf(stderr, "Input Samples Fifo is overflowing!\n");
                    fifo_overflowed += fifo_fill + take - FIFO_COMPLEX;
                    take = FIFO_COMPLEX - fifo_fill;
                }
                std::memcpy(raw.data() + fifo_fill * bytes_per_sample, blockbuf.data(), take * bytes_per_sample);
                fifo_fill += take;
            }
            if (fifo_fill >= FIFO_MIN_COMPLEX || fifo_eof) break;
        }
        // (at the end of the file the reference's loop stops with what is left below the threshold still in the FIFO)
        if (fifo_fill < FIFO_MIN_COMPLEX) return 0;
        const size_t n = fifo_fill;
        fifo_fill = 0;
        ++fifo_calls;
        fifo_min = n < fifo_min ? n : fifo_min;
        fifo_max = n > fifo_max ? n : fifo_max;
        return n;
    };
    std::vector<float> soft(cap);
    std::vector<int8_t> q(cap);
    std::vector<float> mixed(acq ? 2 * max_chunk : 0);
    size_t total_in = 0, total_sym = 0;
    int exit_code = 0;
    for (;;) {
        size_t n = o.fifo ? fifo_chunk() : read_samples(raw.data(), o.block);
        if (n == 0) { std::fprintf(stderr, "EOF\n"); break; }
        if (o.paced && !o.fifo) {
            // CFileFrontend.cpp:36-47: one block per block period
            std::this_thread::sleep_until(t_release);
            t_release += std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                std::chrono::duration<double>((double)n / o.sample_rate));
        }
        size_t nsym = 0;
        if (acq) {
            rc = xrit_acquire_mix(acq, raw.data(), n, type, mixed.data());
            if (rc != XRIT_OK) { std::fprintf(stderr, "mix: %s\n", xrit_last_error()); exit_code = 1; break; }
            rc = xrit_demod_process(chain, mixed.data(), n, XRIT_SAMPLE_FLOATIQ, soft.data(), cap, &nsym);
        } else {
            rc = xrit_demod_process(chain, raw.data(), n, type, soft.data(), cap, &nsym);
        }
        if (rc != XRIT_OK) { std::fprintf(stderr, "process: %s\n", xrit_last_error()); exit_code = 1; break; }
        if (monitor.mon && !monitor.add(soft.data(), nsym)) { exit_code = 1; break; }
        if (o.drop) {
            queue.add(soft.data(), nsym);         // SymbolManager::add: never waits, may drop
        } else {
            rc = xrit_quantize_i8(chain, soft.data(), q.data(), nsym);
            if (rc != XRIT_OK) { std::fprintf(stderr, "quantize: %s\n", xrit_last_error()); exit_code = 1; break; }
            if (!sink.send_all(q.data(), nsym)) { exit_code = 1; break; }
            if ((decode.dec || decode.lk) && !decode.add(q.data(), nsym)) { exit_code = 1; break; }
        }
        if (diag.fd >= 0 && nsym > 0) {
            // the first symbols of the call, complex (stage 4); only what the tap can take is copied back
            std::vector<float> all;
            size_t have = 0;
            if (xrit_demod_read_stage(chain, 4, nullptr, 0, &have) == XRIT_OK && have > 0) {
                all.resize(2 * have);
                if (xrit_demod_read_stage(chain, 4, all.data(), have, &have) == XRIT_OK) diag.add(all.data(), nsym);
            }
            diag.pump();
        }
        total_in += n;
        total_sym += nsym;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    const size_t fill_at_eof = o.drop ? queue.size() : 0;
    if (o.drop) {
        dsp_done.store(true);
        sender.join();
    }
    if (o.stats) {
        xrit_demod_stats st;
        if (xrit_demod_get_stats(chain, &st) == XRIT_OK)
            std::fprintf(stderr, "samples in %zu, symbols out %zu, %.3f s (%.2f Msamples/s incl. file and PCIe)\n",
                         total_in, total_sym, secs, secs > 0 ? total_in / secs * 1e-6 : 0.0);
        if (o.fifo)
            std::fprintf(stderr, "fifo: %zu chunks of %zu .. %zu samples (source blocks of %zu, %d per look), %zu samples lost to overflow\n",
                         fifo_calls, fifo_calls ? fifo_min : 0, fifo_max, o.fifo_block, o.fifo_lag, fifo_overflowed);
        if (o.drop)
            std::fprintf(stderr, "symbol queue: capacity %zu, peak %zu, demodulatorFifoUsage %u %% at end of input (peak %u %%), "
                                 "sent %zu, dropped while full %zu, dropped while disconnected %zu\n",
                         queue.cap, queue.peak, SymbolQueue::usage(fill_at_eof, queue.cap),
                         SymbolQueue::usage(queue.peak, queue.cap), sink.sent, queue.dropped_full,
                         queue.dropped_disconnected);
    }
    sink.close_all();
    decode.close();
    monitor.close();
    std::fclose(in);
    if (acq) xrit_acquire_destroy(acq);
    xrit_demod_destroy(chain);
    return exit_code;
}
