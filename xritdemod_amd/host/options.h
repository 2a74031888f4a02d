// options.h -- the program's command line: Options, usage(), parse().  A refused command line says why on stderr; main
// prints the usage text behind it and exits with status 2.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/xritdemod_amd.h"
#include "jpeg_files.h"
#include "overlay_files.h"
#include "source.h"

struct Options {
    FilesJpegOption files_jpeg;    // --files-jpeg: with --files, image files with compression flag 2 decoded to DIR/STEM.pgm / .ppm (xrit_jpegdec_*)
    OverlayOptions overlay;        // --overlay FILE, --graticule DEG, --overlay-width W: with --products, every toned view also with a map drawn in (xrit_overlay_*)
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

    // the decode chain (stages.h) runs when one of its outputs is asked for
    bool decoding() const { return !decode.empty() || !channels.empty() || !decoder_stats.empty() || !packets.empty() || !files.empty(); }
};

inline void usage()
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
                 "         [--files-jpeg]         (with --files: an image file whose headers say compression 2 carries a baseline JPEG stream in its\n"
                 "                                 data field; when it ends it is decoded on the GPU to ..._{serial}.pgm, or .ppm for three\n"
                 "                                 components; a stream that does not decode writes nothing and gets a line on stderr)\n"
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
                 "         [--overlay FILE] [--graticule DEG] [--overlay-width W]   (with --products: every DIR/<name>.view.pgm is also written\n"
                 "                                 with a map drawn into it on the GPU, as DIR/<name>.view.map.ppm -- the polylines of FILE\n"
                 "                                 (GMT multi-segment text: one `lon lat` pair per line in degrees, a line that is blank or begins\n"
                 "                                 > or # ends a polyline) in opaque yellow (255, 255, 0), and meridians and parallels every DEG\n"
                 "                                 degrees (0.1..90) in cyan (0, 255, 255) at 160 / 255, both with a vertex every 0.05 degrees, W\n"
                 "                                 pixels wide (1..8, default 1); placed by the image navigation record, a canvas without one is\n"
                 "                                 skipped with a line on stderr.  With --project also DIR/<name>.geo.view.map.ppm)\n"
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

// a refused command line: why, on stderr
inline bool refuse(const char *format, ...)
{
    va_list args;
    va_start(args, format);
    std::vfprintf(stderr, format, args);
    va_end(args);
    return false;
}

// --product-tone: linear | equalise | stretch | stretch:LO:HI (per myriad, 0 <= LO < HI <= 10000; plain stretch is 200:9800)
inline bool parse_tone(const char *v, xrit_product_params &p)
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
    return refuse("--product-tone %s: linear, equalise, stretch or stretch:LO:HI with 0 <= LO < HI <= 10000\n", v);
}

// --project-grid LON0:LAT0:STEP:COLUMNS:ROWS
inline bool parse_project_grid(const char *v, xrit_geo_grid &g)
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
    return refuse("--project-grid %s: LON0:LAT0:STEP:COLUMNS:ROWS with STEP > 0, COLUMNS and ROWS 1..%d\n", v, XRIT_GEO_MAX_DIM);
}

// the flags that take one value and store it as it is, and the switches
struct ValueFlag { const char *name; void (*store)(Options &, const char *); };
struct SwitchFlag { const char *name; bool Options::*field; };
const ValueFlag VALUE_FLAGS[] = {
    {"--input", [](Options &o, const char *v) { o.input = v; }},
    {"--format", [](Options &o, const char *v) { o.format = v; }},
    {"--mode", [](Options &o, const char *v) { o.mode = v; }},
    {"--sink", [](Options &o, const char *v) { o.sink = v; }},
    {"--sample-rate", [](Options &o, const char *v) { o.sample_rate = std::atof(v); }},
    {"--decimation", [](Options &o, const char *v) { o.decimation = (unsigned)std::atoi(v); }},
    {"--block", [](Options &o, const char *v) { o.block = (size_t)std::atoll(v); }},
    {"--device", [](Options &o, const char *v) { o.device = std::atoi(v); }},
    {"--connect-tries", [](Options &o, const char *v) { o.connect_tries = std::atoi(v); }},
    {"--diag", [](Options &o, const char *v) { o.diag = v; }},
    {"--queue-symbols", [](Options &o, const char *v) { o.queue_symbols = (size_t)std::atoll(v); }},
    {"--sndbuf", [](Options &o, const char *v) { o.sndbuf = std::atoi(v); }},
    {"--gpus", [](Options &o, const char *v) { o.gpus = std::atoi(v); }},
    {"--fifo-block", [](Options &o, const char *v) { o.fifo_block = (size_t)std::atoll(v); }},
    {"--fifo-lag", [](Options &o, const char *v) { o.fifo_lag = std::atoi(v); }},
    {"--decode", [](Options &o, const char *v) { o.decode = v; }},
    {"--channels", [](Options &o, const char *v) { o.channels = v; }},
    {"--decoder-stats", [](Options &o, const char *v) { o.decoder_stats = v; }},
    {"--packets", [](Options &o, const char *v) { o.packets = v; }},
    {"--files", [](Options &o, const char *v) { o.files = v; }},
    {"--canvas-slots", [](Options &o, const char *v) { o.canvas_slots = (unsigned)std::atoi(v); }},
    {"--canvas-mib", [](Options &o, const char *v) { o.canvas_mib = (size_t)std::atoll(v); }},
    {"--tune", [](Options &o, const char *v) { o.tune = true; o.tune_hz = std::atof(v); }},
    {"--acquire-presum", [](Options &o, const char *v) { o.acquire_presum = (unsigned)std::atoi(v); }},
    {"--monitor", [](Options &o, const char *v) { o.monitor = v; }},
    {"--monitor-block", [](Options &o, const char *v) { o.monitor_block = (unsigned)std::atoi(v); }},
};
const SwitchFlag SWITCH_FLAGS[] = {
    {"--files-decompress", &Options::files_decompress}, {"--canvas", &Options::canvas}, {"--products", &Options::products},
    {"--project", &Options::project}, {"--stream-sync", &Options::stream_sync}, {"--acquire", &Options::acquire},
    {"--fifo", &Options::fifo}, {"--drop", &Options::drop}, {"--paced", &Options::paced}, {"--stats", &Options::stats},
};

// an optional number behind --jpeg / --flywheel: a token that begins with a digit is the number, whole
inline bool optional_number(int argc, char **argv, int &i, const char *name, long lo, long hi, int &out)
{
    if (i + 1 >= argc || argv[i + 1][0] < '0' || argv[i + 1][0] > '9') return true;
    char *end = nullptr;
    const long n = std::strtol(argv[++i], &end, 10);
    if (*end != '\0' || n < lo || n > hi) return refuse("%s %s: %ld..%ld\n", name, argv[i], lo, hi);
    out = (int)n;
    return true;
}

inline bool parse(int argc, char **argv, Options &o)
{
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&]() -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); return nullptr; }
            return argv[++i];
        };
        const char *v = nullptr;
        bool known = false;
        for (const ValueFlag &f : VALUE_FLAGS) {
            if (a != f.name) continue;
            if (!(v = need())) return false;
            f.store(o, v);
            known = true;
        }
        for (const SwitchFlag &f : SWITCH_FLAGS)
            if (a == f.name) known = o.*f.field = true;
        if (known || o.files_jpeg.flag(a)) continue;
        std::string why;
        const int overlay = o.overlay.flag(a, i + 1 < argc ? argv[i + 1] : nullptr, &why);
        if (overlay < 0) return refuse("%s", why.c_str());
        if (overlay > 0) { ++i; continue; }
        if (a == "--product-tone") { if (!(v = need()) || !parse_tone(v, o.product)) return false; o.product_flags = true; }
        else if (a == "--product-factor") {
            if (!(v = need())) return false;
            char *end = nullptr;
            const long f = std::strtol(v, &end, 10);
            if (*v == '\0' || *end != '\0' || f < 1 || f > XRIT_PRODUCT_MAX_FACTOR) return refuse("--product-factor %s: 1..%d\n", v, XRIT_PRODUCT_MAX_FACTOR);
            o.product.factor = (uint32_t)f;
            o.product_flags = true;
        }
        else if (a == "--jpeg") {
            o.jpeg = 90;
            if (!optional_number(argc, argv, i, "--jpeg", 1, 100, o.jpeg)) return false;
        }
        else if (a == "--project-grid") {
            if (!(v = need()) || !parse_project_grid(v, o.project_grid)) return false;
            o.project_flags = o.project_grid_given = true;
        }
        else if (a == "--project-mode") {
            if (!(v = need())) return false;
            if (std::string(v) == "nearest") o.project_mode = XRIT_GEO_NEAREST;
            else if (std::string(v) == "bilinear") o.project_mode = XRIT_GEO_BILINEAR;
            else return refuse("--project-mode %s: nearest or bilinear\n", v);
            o.project_flags = true;
        }
        else if (a == "--flywheel") {
            o.flywheel = 4;                 // parameters.h:41
            o.stream_sync = true;
            if (!optional_number(argc, argv, i, "--flywheel", 1, 255, o.flywheel)) return false;
        }
        else if (a == "--front-exact") {
            o.front_exact = 1;
            if (i + 1 < argc && (std::string(argv[i + 1]) == "1" || std::string(argv[i + 1]) == "2" || std::string(argv[i + 1]) == "-1")) o.front_exact = atoi(argv[++i]);
        }
        else return refuse("unknown option %s\n", a.c_str());
    }
    if (o.fifo && (o.fifo_block < 1 || o.fifo_block > FIFO_COMPLEX || o.fifo_lag < 1 || o.gpus > 1))
        return refuse("--fifo: --fifo-block 1..%zu, --fifo-lag >= 1, one GPU\n", FIFO_COMPLEX);
    if (!o.decode.empty() && (o.drop || o.gpus > 1))
        return refuse("--decode: one GPU, without --drop\n");
    if ((!o.channels.empty() || !o.decoder_stats.empty()) && (o.drop || o.gpus > 1))
        return refuse("--channels / --decoder-stats: one GPU, without --drop\n");
    if (!o.packets.empty() && (o.drop || o.gpus > 1))
        return refuse("--packets: one GPU, without --drop\n");
    if (!o.files.empty() && (o.drop || o.gpus > 1))
        return refuse("--files: one GPU, without --drop\n");
    if (o.stream_sync && !o.decoding())
        return refuse("--stream-sync needs --decode, --channels, --decoder-stats, --packets or --files\n");
    if (o.files_decompress && o.files.empty())
        return refuse("--files-decompress needs --files DIR\n");
    if (const char *why = o.files_jpeg.refused(!o.files.empty())) return refuse("%s", why);
    if (o.canvas && (!o.files_decompress || o.canvas_slots < 1 || o.canvas_slots > XRIT_CANVAS_MAX_SLOTS || o.canvas_mib < 1 || o.canvas_mib > 4096))
        return refuse("--canvas needs --files DIR --files-decompress; --canvas-slots 1..%d, --canvas-mib 1..4096\n", XRIT_CANVAS_MAX_SLOTS);
    if ((o.products && !o.canvas) || (o.product_flags && !o.products))
        return refuse("--products needs --canvas; --product-tone and --product-factor need --products\n");
    if (o.jpeg && !o.products)
        return refuse("--jpeg needs --products\n");
    if (const char *why = o.overlay.refused(o.products)) return refuse("%s", why);
    if ((o.project && !o.canvas) || (o.project_flags && !o.project))
        return refuse("--project needs --canvas; --project-grid and --project-mode need --project\n");
    if ((o.tune || o.acquire) && (o.gpus > 1 || o.format == "u8" || o.acquire_presum < 1 || o.acquire_presum > 64))
        return refuse("--tune / --acquire: one GPU; cf32, s16 or s8 input; --acquire-presum 1..64\n");
    if (!o.monitor.empty() && (o.gpus > 1 || o.monitor_block < 64 || o.monitor_block > 32768 || o.monitor_block % 64))
        return refuse("--monitor: one GPU; --monitor-block a multiple of 64 in 64..32768\n");
    return !o.input.empty() && o.block > 0 && o.decimation >= 1 && o.gpus >= 1;
}
