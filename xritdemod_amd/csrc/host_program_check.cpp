// host_program_check.cpp -- the host program's plain parts (../host/source.h, sinks.h, outputs.h) in a program of their
// own: binary PGM, the canvas name reduction, the journal of a file record, the bound on open packet files, the FIFO
// chunking rule, the replay of what was read ahead, the symbol queue's loss accounting and the int8 quantiser.  It links
// nothing of the library and works in a temporary directory.  Built and run by `make host-program-check` with
// -fsanitize=address,undefined; exits non-zero on the first failed check.
#include <fcntl.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../host/jpeg_files.h"
#include "../host/overlay_files.h"
#include "../host/outputs.h"
#include "../host/sinks.h"
#include "../host/source.h"

namespace fs = std::filesystem;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            return 1;                                                               \
        }                                                                           \
    } while (0)

static std::string slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static size_t count_of(const std::string &text, const std::string &what)
{
    size_t n = 0;
    for (size_t at = text.find(what); at != std::string::npos; at = text.find(what, at + what.size())) ++n;
    return n;
}
static Span span(const std::string &s) { return Span{reinterpret_cast<const uint8_t *>(s.data()), s.size()}; }

// stderr into a file while a case runs that is expected to speak
struct Quiet {
    int saved;
    explicit Quiet(const std::string &path)
    {
        std::fflush(stderr);
        saved = ::dup(2);
        const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        ::dup2(fd, 2);
        ::close(fd);
    }
    ~Quiet()
    {
        std::fflush(stderr);
        ::dup2(saved, 2);
        ::close(saved);
    }
};

// samples of 2 bytes whose value is their index in the stream (mod 65536), read like a file
struct Memory {
    size_t samples, pos = 0;
    size_t operator()(void *dst, size_t count)
    {
        const size_t n = count < samples - pos ? count : samples - pos;
        for (size_t i = 0; i < n; ++i) {
            static_cast<unsigned char *>(dst)[2 * i] = (unsigned char)((pos + i) & 255);
            static_cast<unsigned char *>(dst)[2 * i + 1] = (unsigned char)(((pos + i) >> 8) & 255);
        }
        pos += n;
        return n;
    }
};
static bool holds(const std::vector<unsigned char> &raw, size_t n, size_t first)
{
    for (size_t i = 0; i < n; ++i)
        if (raw[2 * i] != ((first + i) & 255) || raw[2 * i + 1] != (((first + i) >> 8) & 255)) return false;
    return true;
}
static Source fifo_source(size_t samples, size_t block, int lag)
{
    Source s;
    s.reader = Memory{samples};
    s.bytes_per_sample = 2;
    s.fifo = true;
    s.fifo_block = block;
    s.fifo_lag = lag;
    return s;
}

static int check_pgm(const std::string &dir)
{
    // 8 bits, 5 x 3, rows 8 bytes apart
    const uint8_t a[24] = {1, 2, 3, 4, 5, 0xEE, 0xEE, 0xEE, 6, 7, 8, 9, 10, 0xEE, 0xEE, 0xEE, 11, 12, 13, 14, 255, 0xEE, 0xEE, 0xEE};
    CHECK(write_pgm(dir + "/a.pgm", a, 5, 3, 8, 8));
    CHECK(slurp(dir + "/a.pgm") == std::string("P5\n5 3\n255\n\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c\x0d\x0e\xff", 11 + 15));
    // 10 bits, 3 x 2, rows 8 bytes apart: little-endian in, the high byte first out
    const uint8_t b[16] = {0x23, 0x01, 0xFF, 0x03, 0x01, 0x00, 0xEE, 0xEE, 0x00, 0x02, 0x34, 0x02, 0x00, 0x00, 0xEE, 0xEE};
    CHECK(write_pgm(dir + "/b.pgm", b, 3, 2, 8, 10));
    CHECK(slurp(dir + "/b.pgm") == std::string("P5\n3 2\n1023\n\x01\x23\x03\xff\x00\x01\x02\x00\x02\x34\x00\x00", 12 + 12));
    // tight rows, 8 and 12 bits
    const uint8_t c[8] = {9, 8, 7, 6, 5, 4, 3, 2};
    CHECK(write_pgm(dir + "/c.pgm", c, 4, 2, 4, 8));
    CHECK(slurp(dir + "/c.pgm") == std::string("P5\n4 2\n255\n\x09\x08\x07\x06\x05\x04\x03\x02", 11 + 8));
    const uint8_t d[8] = {0xFF, 0x0F, 0x00, 0x01, 0x02, 0x00, 0xCD, 0x0A};
    CHECK(write_pgm(dir + "/d.pgm", d, 2, 2, 4, 12));
    CHECK(slurp(dir + "/d.pgm") == std::string("P5\n2 2\n4095\n\x0f\xff\x01\x00\x00\x02\x0a\xcd", 12 + 8));
    // no rows: the header alone; a directory that is not there: refused
    CHECK(write_pgm(dir + "/e.pgm", c, 0, 0, 0, 8) && slurp(dir + "/e.pgm") == "P5\n0 0\n255\n");
    {
        Quiet q(dir + "/stderr.txt");
        CHECK(!write_pgm(dir + "/nowhere/f.pgm", c, 4, 2, 4, 8));
    }
    return 0;
}

static int check_names()
{
    uint8_t text[64] = {};
    const char with[] = "GOES 16/full\x80" "disk-1_a.lrit\0tail";       // a space, a slash, a byte >= 0x80, a NUL in the middle
    std::memcpy(text, with, sizeof with);
    CHECK(canvas_name(text, sizeof text, 5, 22, 3) == "GOES_16_full_disk-1_a.lrit");
    std::memset(text, 'x', sizeof text);                                // no NUL in the field: all of it, and no further
    CHECK(canvas_name(text, sizeof text, 5, 22, 3) == std::string(64, 'x'));
    std::memset(text, 0, sizeof text);
    CHECK(canvas_name(text, sizeof text, 5, 22, 3) == "vc5_img22_3");
    CHECK(canvas_name(text, sizeof text, 63, 65535, 4000000000ull) == "vc63_img65535_4000000000");
    CHECK(file_stem("D", 5, 42, 7) == "D/vc5_apid42_7");
    return 0;
}

static int check_journal(const std::string &dir)
{
    const std::string bodies[3] = {"abc", "de", "f"};
    const Span abc = span(bodies[0]), de = span(bodies[1]), f = span(bodies[2]);
    const std::string lines_s[3] = {"line0", "LINE1", "l2"};
    const Span lines[3] = {span(lines_s[0]), span(lines_s[1]), span(lines_s[2])};
    // begin, append, end
    std::string stem = file_stem(dir, 1, 10, 0);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS, &abc, false, nullptr, 0) && slurp(stem + ".lrit.part") == "abc");
    CHECK(journal_record(stem, 0, &de, false, nullptr, 0) && slurp(stem + ".lrit.part") == "abcde");
    CHECK(journal_record(stem, XRIT_FILE_ENDS, &f, false, nullptr, 0));
    CHECK(slurp(stem + ".lrit") == "abcdef" && !fs::exists(stem + ".lrit.part") && !fs::exists(stem + ".img.part") && !fs::exists(stem + ".img"));
    // begin, append, abort: nothing is left
    stem = file_stem(dir, 1, 10, 1);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS, &abc, false, nullptr, 0) && journal_record(stem, 0, &de, false, nullptr, 0));
    CHECK(fs::exists(stem + ".lrit.part") && journal_record(stem, XRIT_FILE_ABORTED, nullptr, false, nullptr, 0));
    CHECK(!fs::exists(stem + ".lrit.part") && !fs::exists(stem + ".lrit"));
    // a record that begins and ends in one round
    stem = file_stem(dir, 1, 11, 0);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS | XRIT_FILE_ENDS, &abc, false, nullptr, 0));
    CHECK(slurp(stem + ".lrit") == "abc" && !fs::exists(stem + ".lrit.part"));
    // a record open across two rounds stays .part; what an earlier run left under its name is overwritten where it begins
    stem = file_stem(dir, 2, 12, 0);
    { std::ofstream(stem + ".lrit.part") << "stale bytes of an earlier run"; }
    CHECK(journal_record(stem, XRIT_FILE_BEGINS, &abc, false, nullptr, 0) && slurp(stem + ".lrit.part") == "abc");
    CHECK(journal_record(stem, 0, &de, false, nullptr, 0) && slurp(stem + ".lrit.part") == "abcde" && !fs::exists(stem + ".lrit"));
    CHECK(journal_record(stem, 0, nullptr, false, nullptr, 0) && slurp(stem + ".lrit.part") == "abcde");       // a round without pieces
    // a rice image: the header-only first round has no line yet, a later round has none either
    stem = file_stem(dir, 3, 13, 4);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS, &abc, true, nullptr, 0));
    CHECK(slurp(stem + ".lrit.part") == "abc" && fs::exists(stem + ".img.part") && fs::file_size(stem + ".img.part") == 0);
    CHECK(journal_record(stem, 0, &de, true, lines, 2) && slurp(stem + ".img.part") == "line0LINE1");
    CHECK(journal_record(stem, 0, nullptr, true, lines, 0) && slurp(stem + ".img.part") == "line0LINE1");
    CHECK(journal_record(stem, XRIT_FILE_ENDS, &f, true, lines + 2, 1));
    CHECK(slurp(stem + ".lrit") == "abcdef" && slurp(stem + ".img") == "line0LINE1l2");
    CHECK(!fs::exists(stem + ".lrit.part") && !fs::exists(stem + ".img.part"));
    // ... in one round, and aborted
    stem = file_stem(dir, 3, 13, 5);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS | XRIT_FILE_ENDS, &abc, true, lines, 3) && slurp(stem + ".img") == "line0LINE1l2");
    stem = file_stem(dir, 3, 13, 6);
    CHECK(journal_record(stem, XRIT_FILE_BEGINS, &abc, true, lines, 1) && fs::exists(stem + ".img.part"));
    CHECK(journal_record(stem, XRIT_FILE_ABORTED, &de, true, lines + 1, 1));
    CHECK(!fs::exists(stem + ".lrit.part") && !fs::exists(stem + ".img.part") && !fs::exists(stem + ".lrit") && !fs::exists(stem + ".img"));
    // the per-channel append
    CHECK(append_channel(dir, 7, abc.bytes, 3) && append_channel(dir, 7, de.bytes, 2) && slurp(dir + "/channel_7.bin") == "abcde");
    return 0;
}

static int check_packet_files(const std::string &dir)
{
    // one round's bytes: packet i of the round is the two bytes at 2 i
    std::vector<uint8_t> bytes(2 * 65);
    for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)(i * 7 + 1);
    auto packet = [](int apid, size_t offset, uint8_t crc_ok) {
        xrit_packet d{};
        d.offset = offset;
        d.length = 2;
        d.apid = (uint16_t)apid;
        d.vcid = 9;
        d.crc_ok = crc_ok;
        return d;
    };
    PacketFiles files;
    for (int k = 0; k < 64; ++k) CHECK(files.add(dir, packet(100 + k, 2 * (size_t)k, 1), bytes.data()));
    CHECK(files.files.size() == 64);
    CHECK(files.add(dir, packet(100, 0, 1), bytes.data()) && files.files.size() == 64);       // a key that is open: nothing closes
    CHECK(files.add(dir, packet(164, 128, 1), bytes.data()) && files.files.size() == 1);       // the 65th: all closed, this one open
    for (int k = 0; k < 65; ++k) CHECK(files.add(dir, packet(100 + k, 2 * (size_t)k, 1), bytes.data()));       // reopened for append
    CHECK(files.add(dir, packet(999, 0, 0), bytes.data()));       // a packet whose CRC does not match is not written
    files.close();
    CHECK(files.files.empty() && !fs::exists(dir + "/vc9_apid999.bin"));
    for (int k = 0; k < 65; ++k) {
        const std::string one(reinterpret_cast<const char *>(bytes.data()) + 2 * k, 2);
        CHECK(slurp(dir + "/vc9_apid" + std::to_string(100 + k) + ".bin") == (k == 0 ? one + one + one : one + one));
    }
    return 0;
}

static int check_fifo(const std::string &dir)
{
    CHECK(FIFO_COMPLEX == 524288 && FIFO_MIN_COMPLEX == 32768);
    std::vector<unsigned char> raw(FIFO_COMPLEX * 2);
    {   // a look after every block: each block is above the threshold and goes out alone; the last 3395 samples stay in the FIFO
        Source s = fifo_source(200000, 65535, 1);
        CHECK(s.max_chunk(4096) == 524288);
        CHECK(s.next(raw.data(), 4096) == 65535 && holds(raw, 65535, 0));
        CHECK(s.next(raw.data(), 4096) == 65535 && holds(raw, 65535, 65535));
        CHECK(s.next(raw.data(), 4096) == 65535 && holds(raw, 65535, 131070));
        CHECK(s.next(raw.data(), 4096) == 0 && s.fifo_fill == 3395 && s.fifo_eof);
        CHECK(s.fifo_calls == 3 && s.fifo_min == 65535 && s.fifo_max == 65535 && s.fifo_overflowed == 0);
    }
    {   // a look after every third block: 3 * 65535 at a time; 10185 samples are left at the end
        Source s = fifo_source(600000, 65535, 3);
        CHECK(s.next(raw.data(), 4096) == 196605 && holds(raw, 196605, 0));
        CHECK(s.next(raw.data(), 4096) == 196605 && s.next(raw.data(), 4096) == 196605 && holds(raw, 196605, 393210));
        CHECK(s.next(raw.data(), 4096) == 0 && s.fifo_fill == 10185 && s.fifo_calls == 3 && s.fifo_overflowed == 0);
    }
    {   // small blocks: the source goes on until the threshold is reached, 33 blocks of 1000
        Source s = fifo_source(100000, 1000, 1);
        CHECK(s.next(raw.data(), 4096) == 33000 && s.next(raw.data(), 4096) == 33000 && s.next(raw.data(), 4096) == 33000);
        CHECK(s.next(raw.data(), 4096) == 0 && s.fifo_fill == 1000 && s.fifo_min == 33000);
    }
    {   // nine blocks per look do not fit: 9 * 65535 - 524288 = 65527 samples of the ninth are lost each time, said once
        Source s = fifo_source(2 * 9 * 65535, 65535, 9);
        {
            Quiet q(dir + "/stderr.txt");
            CHECK(s.next(raw.data(), 4096) == 524288 && s.fifo_overflowed == 65527);
            CHECK(holds(raw, 524288, 0));                       // eight whole blocks and the first 8 samples of the ninth
            CHECK(s.next(raw.data(), 4096) == 524288 && s.fifo_overflowed == 131054 && holds(raw, 524288, 589815));
            CHECK(s.next(raw.data(), 4096) == 0 && s.fifo_fill == 0 && s.fifo_calls == 2);
        }
        CHECK(count_of(slurp(dir + "/stderr.txt"), "Input Samples Fifo is overflowing!\n") == 1);
    }
    {   // without --fifo: blocks as asked for, the last one short
        Source s = fifo_source(10000, 65535, 1);
        s.fifo = false;
        CHECK(s.max_chunk(4096) == 4096);
        CHECK(s.next(raw.data(), 4096) == 4096 && s.next(raw.data(), 4096) == 4096 && holds(raw, 4096, 4096));
        CHECK(s.next(raw.data(), 4096) == 1808 && s.next(raw.data(), 4096) == 0);
    }
    return 0;
}

static int check_read_ahead()
{
    std::vector<unsigned char> dst(2 * 100);
    Source s = fifo_source(100, 65535, 1);
    CHECK(s.read_ahead(40) == 40 && s.ahead.size() == 80);
    CHECK(s.read(dst.data(), 10) == 10 && holds(dst, 10, 0));       // ends inside what was read ahead
    CHECK(s.read(dst.data(), 50) == 50 && holds(dst, 50, 10));      // straddles its end: 30 from it, 20 from the reader
    CHECK(s.read(dst.data(), 30) == 30 && holds(dst, 30, 60));      // behind it
    CHECK(s.read(dst.data(), 30) == 10 && holds(dst, 10, 90) && s.read(dst.data(), 30) == 0);
    Source t = fifo_source(100, 65535, 1);                          // an input shorter than what is wanted: all of it, once
    CHECK(t.read_ahead(250) == 100 && t.read(dst.data(), 100) == 100 && holds(dst, 100, 0) && t.read(dst.data(), 1) == 0);
    Source u = fifo_source(100, 65535, 1);                          // a read that ends exactly where the ahead buffer ends
    CHECK(u.read_ahead(40) == 40 && u.read(dst.data(), 40) == 40 && u.read(dst.data(), 5) == 5 && holds(dst, 5, 40));
    return 0;
}

static int check_queue(const std::string &dir)
{
    // the parent expression ((int8_t)(char) of x * 127 clamped to -128 .. 127) on these inputs.  NaN is left out: both
    // comparisons are false, the NaN reaches the cast, and a float-to-integer conversion of NaN is undefined.
    CHECK(quantize_i8(1.0f) == 127 && quantize_i8(-1.0f) == -127);
    CHECK(quantize_i8(1.01f) == 127 && quantize_i8(-1.01f) == -128);
    CHECK(quantize_i8(0.999f) == 126 && quantize_i8(-0.004f) == 0 && quantize_i8(0.0f) == 0 && quantize_i8(-0.5f) == -63);
    CHECK(quantize_i8(1e30f) == 127 && quantize_i8(-1e30f) == -128);

    SymbolQueue queue;
    queue.cap = 10;
    const float sym[8] = {1.0f, -1.0f, 0.5f, -0.004f, 0.999f, 1.01f, -1.01f, 0.25f};
    queue.add(sym, 8);
    CHECK(queue.size() == 8 && queue.peak == 8);
    queue.add(sym, 5);                  // below the capacity when it comes: taken whole, beyond the capacity
    CHECK(queue.size() == 13 && queue.peak == 13 && queue.dropped_full == 0);
    {
        Quiet q(dir + "/stderr.txt");
        queue.add(sym, 4);              // at or beyond it: dropped whole, and counted
        queue.add(sym, 3);
    }
    CHECK(queue.size() == 13 && queue.dropped_full == 7);
    CHECK(count_of(slurp(dir + "/stderr.txt"), "SymbolManager Buffer is full!!! Dropping samples.\n") == 2);
    int8_t out[16] = {};
    CHECK(queue.take(out, 6) == 6 && queue.size() == 7);
    CHECK(out[0] == 127 && out[1] == -127 && out[2] == 63 && out[3] == 0 && out[4] == 126 && out[5] == 127);
    queue.clear_disconnected();
    CHECK(queue.size() == 0 && queue.dropped_disconnected == 7 && queue.peak == 13);
    CHECK(queue.take(out, 6) == 0);
    CHECK(SymbolQueue::usage(13, 10) == 130 && SymbolQueue::usage(50, 100) == 50 && SymbolQueue::usage(0, 100) == 0);
    CHECK(SymbolQueue::usage(300, 100) == 255 && SymbolQueue::usage(5, 0) == 0 && SymbolQueue::usage(1048576, 1048576) == 100);
    return 0;
}

// jpeg_files.h: the option, where the data field begins, PNM
static int check_jpeg_files(const std::string &dir)
{
    FilesJpegOption o;
    CHECK(!o.flag("--files") && !o.flag("--files-jpegs") && !o.on && o.refused(false) == nullptr);
    CHECK(o.flag("--files-jpeg") && o.on && o.refused(true) == nullptr);
    CHECK(std::string(o.refused(false)) == "--files-jpeg needs --files DIR\n");
    size_t n = 7;
    CHECK(data_field(16, 2, 16, &n) == 16 && n == 0);                  // headers only
    CHECK(data_field(25, 2, 1000, &n) == 25 && n == 975);
    CHECK(data_field(25, 1, 1000, &n) == 0 && n == 0 && data_field(25, 0, 1000, &n) == 0 && n == 0);     // the chain was not walked
    CHECK(data_field(1001, 2, 1000, &n) == 0 && n == 0 && data_field(15, 2, 1000, &n) == 0 && n == 0);
    CHECK(pnm_header(1, 9, 7) == "P5\n9 7\n255\n" && pnm_header(3, 65535, 1) == "P6\n65535 1\n255\n");
    CHECK(std::string(pnm_suffix(1)) == ".pgm" && std::string(pnm_suffix(3)) == ".ppm");
    const uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    CHECK(write_pnm(dir + "/a.pgm", px, 1, 3, 2) && slurp(dir + "/a.pgm") == std::string("P5\n3 2\n255\n\x01\x02\x03\x04\x05\x06", 17));
    CHECK(write_pnm(dir + "/a.ppm", px, 3, 2, 2) && slurp(dir + "/a.ppm") == "P6\n2 2\n255\n" + std::string(reinterpret_cast<const char *>(px), 12));
    Quiet quiet(dir + "/stderr_pnm.txt");
    CHECK(!write_pnm(dir + "/none/a.pgm", px, 1, 3, 2));
    return 0;
}

// overlay_files.h: the options, the polyline text
static int check_overlay_files()
{
    OverlayOptions o;
    std::string why;
    CHECK(o.flag("--overlays", "x", &why) == 0 && o.flag("--files", nullptr, &why) == 0 && !o.on() && o.refused(false) == nullptr);
    CHECK(o.flag("--overlay", nullptr, &why) == -1 && why == "--overlay needs a value\n");
    CHECK(o.flag("--overlay", "--graticule", &why) == -1 && why == "--overlay needs a value\n" && o.flag("--graticule", "--products", &why) == -1);
    CHECK(o.flag("--overlay", "", &why) == -1 && why == "--overlay needs a file name\n" && !o.on());
    CHECK(o.flag("--overlay-width", "3", &why) == 1 && o.width == 3 && std::string(o.refused(true)) == "--overlay-width needs --overlay or --graticule\n");
    CHECK(o.flag("--overlay", "coast.txt", &why) == 1 && o.file == "coast.txt" && o.on() && o.refused(true) == nullptr);
    CHECK(std::string(o.refused(false)) == "--overlay / --graticule need --products\n");
    for (const char *bad : {"0", "9", "-1", "3x", "", "1.5"}) CHECK(o.flag("--overlay-width", bad, &why) == -1 && why.find(": 1..8\n") != std::string::npos);
    CHECK(o.width == 3);
    for (const char *bad : {"0", "0.05", "91", "ten", "10d", "nan", ""}) CHECK(o.flag("--graticule", bad, &why) == -1 && why.find(": 0.1..90 degrees\n") != std::string::npos);
    CHECK(o.graticule == 0.0 && o.flag("--graticule", "7.5", &why) == 1 && o.graticule == 7.5);
    OverlayOptions g;
    CHECK(g.flag("--graticule", "90", &why) == 1 && g.on() && g.file.empty() && g.refused(true) == nullptr && g.width == 1);

    std::vector<double> lon, lat;
    CHECK(parse_polylines("", lon, lat) == 0 && lon.empty());
    CHECK(parse_polylines("> first\n-75.5 10\n  -74\t11.25  \r\n\n# note\n1e1 -2.5e0\n>\n3 4", lon, lat) == 0);
    CHECK(lon.size() == 8 && lat.size() == 8);
    CHECK(std::isnan(lon[0]) && std::isnan(lat[0]) && lon[1] == -75.5 && lat[1] == 10.0 && lon[2] == -74.0 && lat[2] == 11.25);
    CHECK(std::isnan(lon[3]) && std::isnan(lon[4]) && lon[5] == 10.0 && lat[5] == -2.5 && std::isnan(lat[6]) && lon[7] == 3.0 && lat[7] == 4.0);
    CHECK(parse_polylines("1 2\n", lon, lat) == 0 && lon.size() == 1);            // nothing behind the last newline
    CHECK(parse_polylines("1 2\n\n", lon, lat) == 0 && lon.size() == 2 && std::isnan(lon[1]));
    CHECK(parse_polylines("1 2\n3\n", lon, lat) == 2 && parse_polylines("1 2 3", lon, lat) == 1 && parse_polylines("1,2", lon, lat) == 1);
    CHECK(parse_polylines("1 2\n>\nlon lat\n", lon, lat) == 3 && parse_polylines("1 nan", lon, lat) == 1 && parse_polylines("inf 2", lon, lat) == 1);
    CHECK(parse_polylines("1 2x", lon, lat) == 1 && parse_polylines("\n\n\n4 5 # east", lon, lat) == 4);
    CHECK(OVERLAY_COAST_RGBA[3] == 255 && OVERLAY_GRATICULE_RGBA[2] == 255 && OVERLAY_DENSIFY_DEG == 0.05);
    return 0;
}

int main()
{
    char pattern[] = "/tmp/host_program_check.XXXXXX";
    const char *made = ::mkdtemp(pattern);
    CHECK(made != nullptr);
    const std::string dir = made;
    const int rc = check_pgm(dir) || check_names() || check_journal(dir) || check_packet_files(dir) || check_fifo(dir) ||
                   check_read_ahead() || check_queue(dir) || check_jpeg_files(dir) || check_overlay_files();
    fs::remove_all(dir);
    if (rc == 0) std::printf("host_program_check: ok\n");
    return rc;
}
