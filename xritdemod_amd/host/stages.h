// stages.h -- the decode chain behind the soft symbols, one small struct per stage of the library: frame search (fixed
// windows, the stream frame synchroniser or the frame lock), frame decoder, demultiplexer, packets, files, images, canvas,
// products, JPEG, projection; and the link monitor next to it.  Each stage owns its handle (released by scope), its buffers
// and its counters, and report() prints its line on stderr.  DecodeChain is the sequence of them, written out.
//
// The decoder's steps per frame (decoder/src/newdecoder.cpp:218-359) on the quantised symbols: whole 16384-symbol windows go
// through the correlator, the frame fix (HRIT: word forced to 0, NRZ-M takes the phase) and the frame decoder; the symbols
// from the first window whose frame is not complete yet wait for the next round.  --channels / --decoder-stats add the
// channel demultiplexer behind the decoder (:309-395): ChannelWriter's files and the Statistics_st stream, from the
// correlator's hits as it returned them.  --packets adds the packet assembler behind the demultiplexer: the channels' rows
// go back to the device and come out as CRC-checked space packets.  --files adds the file assembler behind that (and, with
// --files-decompress, the image stage: the lines of rice-coded image files).
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <memory>

#include "options.h"
#include "outputs.h"

template <class T, auto Destroy>
struct Handle {
    T *p = nullptr;
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ~Handle() { if (p) Destroy(p); }
    operator T *() const { return p; }
};

// the library refused: its reason, and false
inline bool library_error(const char *prefix = "xritdemod_amd")
{
    std::fprintf(stderr, "%s: %s\n", prefix, xrit_last_error());
    return false;
}
inline bool fail(const char *what)
{
    std::fprintf(stderr, "decode: %s: %s\n", what, xrit_last_error());
    return false;
}
inline bool make_dir(const std::string &dir, const char *flag)
{
    if (::mkdir(dir.c_str(), 0755) == 0 || errno == EEXIST) return true;
    std::perror(flag);
    return false;
}
inline void report_framer(const xrit_framer_counters &c)
{
    std::fprintf(stderr, "sync: %llu symbols, %llu frames, %llu chunks dropped, %llu resynchronisations, %llu symbols left\n",
                 (unsigned long long)c.symbols, (unsigned long long)c.frames, (unsigned long long)c.dropped_chunks,
                 (unsigned long long)c.resyncs, (unsigned long long)c.carry);
}

constexpr size_t FRAME = 16384, VCDU = 892;

// a round's rows, as the frame search and the frame decoder leave them for the stages behind
struct Rows {
    std::vector<xrit_sync_hit> hits, raw_hits;      // raw: the demux takes the phase as the correlator found it
    std::vector<int8_t> frames;
    std::vector<uint8_t> valid, modes, cadu, block;
    std::vector<uint64_t> starts;
    std::vector<xrit_frame_info> info;

    void found(size_t cap)
    {
        hits.resize(cap);
        frames.resize(cap * FRAME);
        valid.resize(cap);
        starts.resize(cap);
    }
    void decoded(size_t cap)
    {
        cadu.resize(cap * 1024);
        block.resize(cap * 1020);
        info.resize(cap);
    }
};

// frames by correlating fixed windows: the symbols wait here until their window's frame is complete
struct Windows {
    static constexpr uint32_t MIN_CORRELATION = 46;     // MINCORRELATIONBITS (parameters.h:31)
    std::vector<int8_t> pending;

    bool find(Rows &r, const int8_t *sym, size_t n, bool hrit, int device, size_t &take)
    {
        take = 0;
        pending.insert(pending.end(), sym, sym + n);
        const size_t nw = pending.size() / FRAME;
        if (nw == 0) return true;
        // newdecoder.cpp:21-24
        const uint64_t words[2] = {hrit ? 0xfc4ef4fd0cc2df89ull : 0xfca2b63db00d9794ull, hrit ? 0x25010b02f33d2076ull : 0x035d49c24ff2686bull};
        r.hits.resize(nw);
        r.frames.resize(nw * FRAME);
        r.valid.resize(nw);
        if (xrit_sync_correlate(pending.data(), nw * FRAME, words, 2, FRAME, r.hits.data(), device) != XRIT_OK) return fail("correlate");
        take = nw;                  // windows decoded this round
        r.raw_hits.assign(r.hits.begin(), r.hits.end());
        for (size_t f = 0; f < nw; ++f) {
            if (hrit) r.hits[f].word = 0;
            if (r.hits[f].correlation >= MIN_CORRELATION && f * FRAME + r.hits[f].position + FRAME > pending.size()) { take = f; break; }
        }
        if (take == 0) return true;
        if (xrit_sync_fix_frames(pending.data(), pending.size(), r.hits.data(), FRAME, MIN_CORRELATION, r.frames.data(), r.valid.data(),
                                 device) != XRIT_OK)
            return fail("fix frames");
        pending.erase(pending.begin(), pending.begin() + (std::ptrdiff_t)(take * FRAME));       // (the frames are copies)
        return true;
    }
};

// --stream-sync: the framer keeps the cursor and the unconsumed symbols on the device; its rows are what the fixed windows'
// correlate + fix give, found chunk by chunk from where the last frame ended
struct Framer {
    Handle<xrit_framer, xrit_framer_destroy> fr;

    bool find(Rows &r, const int8_t *sym, size_t n, size_t &take)
    {
        r.found(xrit_framer_rows(fr, n));
        const int got = xrit_framer_push(fr, sym, n, r.frames.data(), r.valid.data(), r.hits.data(), r.starts.data());
        if (got < 0) return fail("frame synchroniser");
        take = (size_t)got;
        r.raw_hits.assign(r.hits.begin(), r.hits.begin() + (std::ptrdiff_t)take);
        return true;
    }
    void report() const
    {
        xrit_framer_counters c{};
        if (xrit_framer_stats(fr, &c) == XRIT_OK) report_framer(c);
    }
};

// --flywheel: the lock's rows are the framer's and the decoder's at once
struct Lock {
    Handle<xrit_lock, xrit_lock_destroy> lk;

    bool find(Rows &r, const int8_t *sym, size_t n, size_t &take)
    {
        const size_t cap = xrit_lock_rows(lk, n);
        r.found(cap);
        r.modes.resize(cap);
        r.decoded(cap);
        const int got = xrit_lock_push(lk, sym, n, r.frames.data(), r.valid.data(), r.hits.data(), r.starts.data(), r.modes.data(),
                                       r.cadu.data(), r.block.data(), r.info.data());
        if (got < 0) return fail("frame lock");
        take = (size_t)got;
        r.raw_hits.assign(r.hits.begin(), r.hits.begin() + (std::ptrdiff_t)take);
        return true;
    }
    void report() const
    {
        xrit_lock_counters c{};
        if (xrit_lock_stats(lk, &c) != XRIT_OK) return;
        report_framer(c.framer);
        std::fprintf(stderr, "lock: %llu chunks kept at position 0 of the short range, %llu missed there, %llu rechecks, "
                             "%llu chunks that hung on the frame before, %llu rounds in %llu calls\n",
                     (unsigned long long)c.short_kept, (unsigned long long)c.short_missed, (unsigned long long)c.rechecks,
                     (unsigned long long)c.sensitive_chunks, (unsigned long long)c.rounds, (unsigned long long)c.framer.calls);
    }
};

// the frame decoder (not with --flywheel), the counts over the decoded frames and --decode's file of good VCDUs
struct Decoder {
    Handle<xrit_decoder, xrit_decoder_destroy> dec;
    File out;
    size_t n_frames = 0, n_ok = 0, n_dropped = 0, rs_corrections = 0, viterbi_errors = 0;

    bool decode(Rows &r, size_t take)
    {
        r.decoded(take);
        if (xrit_decoder_decode(dec, r.frames.data(), r.valid.data(), take, r.cadu.data(), r.block.data(), r.info.data()) != XRIT_OK)
            return fail("decode");
        return true;
    }
    bool account(const Rows &r, size_t take)
    {
        for (size_t f = 0; f < take; ++f) {
            const xrit_frame_info &i = r.info[f];
            if (!i.valid) continue;
            ++n_frames;
            viterbi_errors += i.viterbi_errors;
            if (!i.ok) { ++n_dropped; continue; }
            ++n_ok;
            for (int k = 0; k < 4; ++k) rs_corrections += i.rs_errors[k] > 0 ? (size_t)i.rs_errors[k] : 0;
            if (out.f && std::fwrite(r.block.data() + f * 1020, 1, VCDU, out.f) != VCDU) { std::perror("decode output"); return false; }
        }
        return true;
    }
    void report() const
    {
        std::fprintf(stderr, "decode: %zu frames, %zu ok, %zu dropped, %zu RS corrections, mean Viterbi errors %.2f\n", n_frames, n_ok,
                     n_dropped, rs_corrections, n_frames ? (double)viterbi_errors / (double)n_frames : 0.0);
    }
};

// ChannelWriter::writeChannel per good frame (newdecoder.cpp:356-360) and the statistics record of every valid frame
struct Demux {
    Handle<xrit_demux, xrit_demux_destroy> dm;
    std::string channel_dir;
    File stats_out;
    std::vector<uint8_t> vcdu, wire;
    std::vector<xrit_frame_stats> records;
    xrit_decoder_stats stats{};
    uint32_t off[65];               // the round's rows per channel: channel v's are vcdu[off[v] .. off[v + 1])

    bool process(const Rows &r, size_t take)
    {
        vcdu.resize(take * VCDU);
        records.resize(take);
        const xrit_decoder_stats start = stats;
        if (xrit_demux_process(dm, r.raw_hits.data(), r.cadu.data(), r.block.data(), r.info.data(), take, vcdu.data(), off,
                               records.data()) != XRIT_OK || xrit_demux_stats(dm, &stats) != XRIT_OK)
            return fail("demux");
        for (int v = 0; !channel_dir.empty() && v < 64; ++v)
            if (off[v + 1] != off[v] && !append_channel(channel_dir, v, vcdu.data() + (size_t)off[v] * VCDU, (size_t)(off[v + 1] - off[v]) * VCDU))
                return false;
        if (stats_out.f) {
            wire.resize(take * XRIT_STATISTICS_WIRE_BYTES);
            const int n = xrit_demux_expand(&start, records.data(), take, wire.data());
            if (n < 0) return fail("statistics");
            const size_t bytes = (size_t)n * XRIT_STATISTICS_WIRE_BYTES;
            if (std::fwrite(wire.data(), 1, bytes, stats_out.f) != bytes) { std::perror("decoder statistics output"); return false; }
        }
        return true;
    }
    void report() const
    {
        std::fprintf(stderr, "demux: lost packets %lld (", (long long)stats.lost_packets);
        const char *sep = "";
        for (int v = 0; v < 64; ++v) {
            if (stats.received[v] < 0) continue;
            std::fprintf(stderr, "%svcid %d: %lld of %lld", sep, v, (long long)stats.lost[v], (long long)stats.received[v]);
            sep = ", ";
        }
        std::fprintf(stderr, ")\n");
    }
};

// the space packets of a round's rows; what has begun and not ended waits on the device for the next round
struct Packets {
    Handle<xrit_packets, xrit_packets_destroy> pk;
    std::string dir;                // --packets, empty: the packets go to the file assembler only
    std::unique_ptr<uint8_t[]> bytes;
    std::unique_ptr<xrit_packet[]> desc;
    size_t bytes_cap = 0, desc_cap = 0;
    PacketFiles written;
    xrit_packets_summary summary{};
    uint32_t off[65];

    bool process(const Demux &d)
    {
        const size_t rows = d.off[64], need_bytes = XRIT_PACKETS_MAX_BYTES(rows), need_desc = 127 * rows + 64;
        if (need_bytes > bytes_cap) { bytes.reset(new uint8_t[need_bytes]); bytes_cap = need_bytes; }
        if (need_desc > desc_cap) { desc.reset(new xrit_packet[need_desc]); desc_cap = need_desc; }
        if (xrit_packets_process(pk, d.vcdu.data(), d.off, bytes.get(), bytes_cap, desc.get(), desc_cap, off, &summary) != XRIT_OK)
            return fail("packets");
        for (size_t i = 0; !dir.empty() && i < summary.packets; ++i)
            if (!written.add(dir, desc[i], bytes.get())) return false;
        return true;
    }
    void report() const
    {
        std::fprintf(stderr, "packets: %llu emitted, %llu CRC failures, %llu discarded, %llu fill\n", (unsigned long long)summary.total_packets,
                     (unsigned long long)summary.crc_failures, (unsigned long long)summary.discarded, (unsigned long long)summary.fill_packets);
    }
};

// the files of a round's packets: records, their pieces and their bytes; what is open waits on the device (the key's state)
struct Files {
    Handle<xrit_files, xrit_files_destroy> fa;
    std::string dir;
    std::vector<uint8_t> bytes;
    std::vector<xrit_file_piece> pieces;
    std::vector<xrit_file_record> recs;
    xrit_files_summary summary{};

    bool process(const Packets &p)
    {
        const size_t n = p.off[64];
        bytes.resize(XRIT_FILES_MAX_BYTES(p.summary.bytes) + 1);
        pieces.resize(XRIT_FILES_MAX_PIECES(n) + 1);
        recs.resize(XRIT_FILES_MAX_FILES(n) + 1);
        if (xrit_files_process(fa, p.bytes.get(), p.summary.bytes, p.desc.get(), p.off, bytes.data(), bytes.size(), pieces.data(),
                               pieces.size(), recs.data(), recs.size(), &summary) != XRIT_OK)
            return fail("files");
        return true;
    }
    void report() const
    {
        std::fprintf(stderr, "files: %llu begun, %llu completed, %llu aborted, %llu pieces, %llu bad packets, %llu gaps, %llu orphans\n",
                     (unsigned long long)summary.files_begun, (unsigned long long)summary.files_completed,
                     (unsigned long long)summary.files_aborted, (unsigned long long)summary.total_pieces,
                     (unsigned long long)summary.bad_packets, (unsigned long long)summary.seq_gaps, (unsigned long long)summary.orphans);
    }
};

// --files-decompress: every Rice-coded line of a round's records in one call; which images are open waits on the device
struct Images {
    Handle<xrit_images, xrit_images_destroy> im;
    std::vector<uint8_t> img;
    std::vector<xrit_image_line> lines;
    std::vector<xrit_image_file> files;     // the stage's verdict per record of the round
    xrit_images_summary summary{};
    std::vector<Span> spans;
    size_t rice_lines = 0, rice_faults = 0;

    bool process(const Files &f)
    {
        size_t bound = 0;           // every piece of a record a line of the record's width, padded
        for (size_t i = 0; i < f.summary.files; ++i)
            bound += (size_t)f.recs[i].n_pieces * (((size_t)f.recs[i].columns * (f.recs[i].bits_per_pixel <= 8 ? 1 : 2) + 3) & ~(size_t)3);
        img.resize(bound + 1);
        lines.resize(f.summary.pieces + 1);
        files.resize(f.summary.files + 1);
        if (xrit_images_process(im, f.bytes.data(), f.summary.bytes, f.pieces.data(), f.summary.pieces, f.recs.data(), f.summary.files,
                                &f.summary, img.data(), bound, lines.data(), f.summary.pieces, files.data(), &summary) != XRIT_OK)
            return fail("images");
        return true;
    }
    // record i's decoded lines of this round, counted
    // (the stage pads every line to a multiple of 4 bytes; the .img holds them back to back)
    const std::vector<Span> &lines_of(size_t i)
    {
        const xrit_image_file &g = files[i];
        spans.clear();
        for (size_t k = 0; k < g.n_lines; ++k) spans.push_back(Span{img.data() + lines[g.first_line + k].offset, lines[g.first_line + k].length});
        if (g.n_lines) {
            rice_lines += g.n_lines;
            rice_faults += g.faults;
        }
        return spans;
    }
    void report() const { std::fprintf(stderr, "rice: %zu lines decoded, %zu faulted\n", rice_lines, rice_faults); }
};

// --canvas: a round's lines into their images' canvases
struct Canvas {
    Handle<xrit_canvas, xrit_canvas_destroy> cv;
    unsigned n_slots = 0;
    std::vector<xrit_canvas_file> files;
    std::vector<xrit_canvas_slot> slots;
    std::vector<uint8_t> pixels;
    xrit_canvas_summary summary{};
    size_t written = 0;

    bool process(const Files &f, const Images &g)
    {
        files.resize(f.summary.files + 1);
        if (xrit_canvas_process(cv, f.bytes.data(), f.summary.bytes, f.pieces.data(), f.summary.pieces, f.recs.data(), f.summary.files,
                                &f.summary, g.img.data(), g.summary.bytes, g.lines.data(), g.summary.lines, g.files.data(), &g.summary,
                                files.data(), slots.data(), &summary) != XRIT_OK)
            return fail("canvas");
        return true;
    }
    void report(size_t partial) const
    {
        std::fprintf(stderr, "canvas: %llu images begun, %zu written (%zu of them partial), %llu lines placed, %llu clipped, "
                             "%llu segment files refused\n",
                     (unsigned long long)summary.canvases_begun, written, partial, (unsigned long long)summary.lines_placed,
                     (unsigned long long)summary.lines_clipped,
                     (unsigned long long)(summary.bad_segment + summary.too_large + summary.duplicate + summary.overlap + summary.no_slot +
                                          summary.no_placement));
    }
};

// --jpeg: one 8-bit image in device memory as a JPEG file, a restart marker per row of blocks; a file longer than the pixels
// (noise at a high quality) takes a second call with the room the first one asked for
struct Jpeg {
    Handle<xrit_jpeg, xrit_jpeg_destroy> jp;
    int quality = 0;
    std::vector<uint8_t> file;
    size_t written = 0, bytes = 0;

    bool write(const std::string &path, const uint8_t *d_pixels, uint32_t columns, uint32_t rows)
    {
        if (!d_pixels || !columns || !rows) return true;
        if (xrit_jpeg_set_quality(jp, (uint32_t)quality, (columns + 7) / 8) != XRIT_OK) return fail("jpeg");
        const xrit_product_image image{d_pixels, columns, rows, columns, 8};
        xrit_jpeg_result result{};
        file.resize((size_t)columns * rows + 4096);
        int rc = xrit_jpeg_encode_resident(jp, &image, 1, file.data(), file.size(), &result);
        if (rc == XRIT_E_CAPACITY) {
            file.resize((size_t)result.size);
            rc = xrit_jpeg_encode_resident(jp, &image, 1, file.data(), file.size(), &result);
        }
        if (rc != XRIT_OK) return fail("jpeg");
        if (!write_file(path, "wb", file.data(), (size_t)result.size)) return false;
        ++written;
        bytes += (size_t)result.size;
        return true;
    }
    void report() const { std::fprintf(stderr, "jpeg: %zu files of quality %d, %zu bytes\n", written, quality, bytes); }
};

// --files-jpeg: the data field of a finished STEM.lrit whose headers say compression 2, decoded to STEM.pgm / STEM.ppm
struct JpegFiles {
    Handle<xrit_jpegdec, xrit_jpegdec_destroy> jd;
    std::vector<uint8_t> file, pixels;
    size_t written = 0, refused = 0;

    bool write(const std::string &stem, const xrit_file_record &r)
    {
        FILE *f = std::fopen((stem + ".lrit").c_str(), "rb");
        if (!f) { std::perror((stem + ".lrit").c_str()); return false; }
        file.resize((size_t)(r.file_offset + r.length));
        const bool whole = std::fread(file.data(), 1, file.size(), f) == file.size();
        std::fclose(f);
        if (!whole) { std::perror((stem + ".lrit").c_str()); return false; }
        size_t n = 0;
        const size_t at = data_field(r.header_length, r.header_state, file.size(), &n);
        xrit_jpegdec_info info{};
        info.status = XRIT_JPEGDEC_DAMAGED;
        if (n && xrit_jpegdec_header(file.data() + at, n, &info) != XRIT_OK) return fail("files-jpeg");
        xrit_jpegdec_record rec{};
        rec.status = info.status;
        if (info.status == XRIT_JPEGDEC_OK) {
            struct { uint64_t offset; uint32_t length, pad; } item{0, (uint32_t)n, 0};
            xrit_jpegdec_summary summary{};
            pixels.resize(((size_t)info.columns * info.rows * info.components + 3) & ~(size_t)3);
            if (xrit_jpegdec_decode(jd, file.data() + at, n, &item, sizeof item, 1, pixels.data(), pixels.size(), &rec, &summary) != XRIT_OK)
                return fail("files-jpeg");
        }
        if (rec.status != XRIT_JPEGDEC_OK) {
            ++refused;
            std::fprintf(stderr, "files-jpeg: %s.lrit: status %u, nothing written\n", stem.c_str(), rec.status);
            return true;
        }
        ++written;
        return write_pnm(stem + pnm_suffix(rec.components), pixels.data(), rec.components, rec.columns, rec.rows);
    }
    void report() const { std::fprintf(stderr, "files-jpeg: %zu images written, %zu streams refused\n", written, refused); }
};

// --products: a slot's pixels toned and reduced where they lie; the two products are what is downloaded
struct Products {
    Handle<xrit_product, xrit_product_destroy> pr;
    xrit_product_params params{};
    std::vector<uint8_t> tone, small;
    size_t written = 0, fallbacks = 0;

    bool write(const Canvas &c, unsigned s, const xrit_canvas_slot &info, const std::string &stem, Jpeg &jpeg)
    {
        if (!info.max_column || !info.max_row) return true;
        xrit_product_image image{nullptr, info.max_column, info.max_row, info.pitch, info.bits};
        if (xrit_canvas_pixels_device(c.cv, s, &image.d_pixels) != XRIT_OK) return fail("canvas pixels");
        const uint32_t f = params.factor, small_columns = (info.max_column + f - 1) / f, small_rows = (info.max_row + f - 1) / f;
        tone.resize((size_t)info.max_column * info.max_row);
        small.resize((size_t)small_columns * small_rows);
        xrit_product_summary sum{};
        if (xrit_product_process_resident(pr, &image, &params, nullptr, nullptr, nullptr, tone.data(), small.data(), &sum) != XRIT_OK)
            return fail("products");
        fallbacks += sum.fallback;
        if (!write_pgm(stem + ".view.pgm", tone.data(), sum.tone_columns, sum.tone_rows, sum.tone_columns, 8) ||
            !write_pgm(stem + ".thumb.pgm", small.data(), sum.small_columns, sum.small_rows, sum.small_columns, 8))
            return false;
        ++written;
        if (!jpeg.jp) return true;
        // --jpeg: both encoded where the product call left them on the device
        const uint8_t *d_tone = nullptr, *d_small = nullptr;
        if (xrit_product_outputs_device(pr, &d_tone, &d_small) != XRIT_OK) return fail("product outputs");
        return jpeg.write(stem + ".view.jpg", d_tone, sum.tone_columns, sum.tone_rows) &&
               jpeg.write(stem + ".thumb.jpg", d_small, sum.small_columns, sum.small_rows);
    }
    void report() const
    {
        std::fprintf(stderr, "products: %zu canvases toned and reduced %u times, %zu of them by the linear fallback\n", written,
                     params.factor, fallbacks);
    }
};

// --project: a slot's pixels resampled where they lie; the projected image is what is downloaded
struct Projection {
    Handle<xrit_geo, xrit_geo_destroy> geo;
    struct SlotNav { int state = 0; xrit_geo_nav nav{}; };      // 0: no file at (0, 0) yet; 1: its record parsed; 2: it did not
    std::vector<SlotNav> nav;       // per canvas slot
    xrit_geo_grid grid{};
    bool grid_given = false, grid_set = false;
    double grid_lon = 0.0;          // the sub-satellite longitude the tables in effect were made for
    uint32_t mode = XRIT_GEO_BILINEAR;
    std::vector<uint8_t> out, tone;
    size_t projected = 0, skipped = 0;
    bool wrote_view = false;        // the last write() left the projected image's toned view in `tone`

    // a canvas's navigation is that of its segment file at line 0, column 0 -- the record in that file's first piece
    void note_navigation(const Files &f, const Canvas &c)
    {
        for (size_t i = 0; i < f.summary.files; ++i) {
            const xrit_file_record &r = f.recs[i];
            const xrit_canvas_file &p = c.files[i];
            if (!(r.flags & XRIT_FILE_BEGINS) || p.reason != XRIT_CANVAS_PLACED || p.slot < 0 || (unsigned)p.slot >= c.n_slots ||
                p.start_line || p.start_column || !r.n_pieces)
                continue;
            const xrit_file_piece &first = f.pieces[r.first_piece];
            SlotNav &n = nav[(unsigned)p.slot];
            n.state = xrit_geo_parse_navigation(f.bytes.data() + first.offset, first.length, &n.nav) == XRIT_OK ? 1 : 2;
        }
    }
    bool write(const Canvas &c, unsigned s, const xrit_canvas_slot &info, const std::string &stem, Products &products)
    {
        wrote_view = false;
        if (!info.max_column || !info.max_row) return true;
        const SlotNav &n = nav[s];
        if (n.state != 1) {
            std::fprintf(stderr, "project: %s: %s, not projected\n", stem.c_str(),
                         n.state ? "the image navigation record of its file at line 0, column 0 does not parse" : "no segment file at line 0, column 0");
            ++skipped;
            return true;
        }
        if (!grid_set || grid_lon != n.nav.sub_lon_deg) {           // once per geometry
            xrit_geo_grid g = grid;
            if (!grid_given) {      // the earth's disc as the satellite sees it: 81.3 degrees either way
                g.columns = g.rows = 3253;
                g.lon0_deg = n.nav.sub_lon_deg - 81.3;
                g.lat0_deg = 81.3;
            }
            if (xrit_geo_set_grid(geo, &g, n.nav.sub_lon_deg) != XRIT_OK) return fail("project grid");
            grid = g;
            grid_set = true;
            grid_lon = n.nav.sub_lon_deg;
        }
        xrit_product_image image{nullptr, info.max_column, info.max_row, info.pitch, info.bits};
        if (xrit_canvas_pixels_device(c.cv, s, &image.d_pixels) != XRIT_OK) return fail("canvas pixels");
        const uint32_t columns = grid.columns, rows = grid.rows, width = info.bits <= 8 ? 1 : 2;
        out.resize((size_t)columns * rows * width);
        xrit_geo_summary summary{};
        if (xrit_geo_project_resident(geo, &n.nav, &image, mode, out.data(), columns * width, &summary) != XRIT_OK) return fail("project");
        if (!write_pgm(stem + ".geo.pgm", out.data(), columns, rows, (size_t)columns * width, info.bits)) return false;
        ++projected;
        if (!products.pr) return true;
        // --products: the projected image toned like the canvas
        const xrit_product_image flat{out.data(), columns, rows, columns * width, info.bits};
        tone.resize((size_t)columns * rows);
        xrit_product_summary toned{};
        if (xrit_product_process(products.pr, &flat, &products.params, nullptr, nullptr, nullptr, tone.data(), nullptr, &toned) != XRIT_OK)
            return fail("products of the projection");
        wrote_view = write_pgm(stem + ".geo.view.pgm", tone.data(), columns, rows, columns, 8);
        return wrote_view;
    }
    void report() const
    {
        std::fprintf(stderr, "project: %zu canvases projected onto %u x %u (%s), %zu skipped\n", projected, grid.columns, grid.rows,
                     mode == XRIT_GEO_NEAREST ? "nearest" : "bilinear", skipped);
    }
};

// --overlay / --graticule: coastlines (layer 0) and graticule (layer 1) drawn into a mask and blended into a toned view
// where the product stage left it on the device; the vertices are placed by the canvas's navigation record (the scan
// geometry) or on the projection's grid.  The vertex lists are fixed for the run, so each of the two kinds of view has a
// handle of its own that keeps its mask on the device (xrit_overlay_mask_device): it is drawn again only when the
// geometry or the size of the view changes.
struct MapOverlay {
    struct Kind {
        Handle<xrit_overlay, xrit_overlay_destroy> ov;
        std::string key;            // the geometry and size the mask on the device was drawn for; empty: none
        uint32_t pitch = 0;
    };
    Kind kinds[2];                  // 0: the scan geometry, 1: the grid
    std::vector<double> lon[2], lat[2];             // per layer, densified; NaN: a break
    unsigned width = 1;
    xrit_overlay_style styles[XRIT_OVERLAY_LAYERS] = {};
    std::vector<double> quads;
    std::vector<xrit_geo_point> points;
    std::vector<uint8_t> mask, out;
    size_t written = 0, skipped = 0, drawn = 0;

    bool on() const { return (bool)kinds[0].ov; }
    bool open(int device)
    {
        return xrit_overlay_create(&kinds[0].ov.p, device) == XRIT_OK && xrit_overlay_create(&kinds[1].ov.p, device) == XRIT_OK;
    }
    bool load(const OverlayOptions &o)
    {
        width = o.width;
        for (auto &s : styles) s = xrit_overlay_style{255, 255, 255, 255};
        styles[0] = xrit_overlay_style{OVERLAY_COAST_RGBA[0], OVERLAY_COAST_RGBA[1], OVERLAY_COAST_RGBA[2], OVERLAY_COAST_RGBA[3]};
        styles[1] = xrit_overlay_style{OVERLAY_GRATICULE_RGBA[0], OVERLAY_GRATICULE_RGBA[1], OVERLAY_GRATICULE_RGBA[2], OVERLAY_GRATICULE_RGBA[3]};
        std::vector<double> raw_lon, raw_lat;
        if (!o.file.empty()) {
            std::vector<unsigned char> text;
            FILE *f = std::fopen(o.file.c_str(), "rb");
            if (!f) { std::perror(o.file.c_str()); return false; }
            unsigned char buf[65536];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
            std::fclose(f);
            const size_t bad = parse_polylines(std::string(text.begin(), text.end()), raw_lon, raw_lat);
            if (bad) { std::fprintf(stderr, "--overlay %s: line %zu is not `lon lat`\n", o.file.c_str(), bad); return false; }
            if (!densify(raw_lon, raw_lat, 0)) return false;
        }
        if (o.graticule > 0.0) {
            size_t n = 0;
            const double vertex = o.graticule < 1.0 ? o.graticule : 1.0;
            if (xrit_overlay_graticule(o.graticule, vertex, nullptr, nullptr, 0, &n) != XRIT_E_CAPACITY) return fail("graticule");
            raw_lon.resize(n);
            raw_lat.resize(n);
            if (xrit_overlay_graticule(o.graticule, vertex, raw_lon.data(), raw_lat.data(), n, &n) != XRIT_OK) return fail("graticule");
            if (!densify(raw_lon, raw_lat, 1)) return false;
        }
        return true;
    }
    bool densify(const std::vector<double> &a, const std::vector<double> &b, int layer)
    {
        size_t n = 0;
        const int rc = xrit_overlay_densify(a.data(), b.data(), a.size(), OVERLAY_DENSIFY_DEG, nullptr, nullptr, 0, &n);
        if (rc != XRIT_OK && rc != XRIT_E_CAPACITY) return fail("overlay vertices");
        lon[layer].resize(n);
        lat[layer].resize(n);
        return !n || xrit_overlay_densify(a.data(), b.data(), a.size(), OVERLAY_DENSIFY_DEG, lon[layer].data(), lat[layer].data(), n, &n) == XRIT_OK ||
               fail("overlay vertices");
    }
    // both layers into the kind's mask of a columns x rows image -- nav: through the scan geometry; grid: on that grid, with
    // max_jump half its width
    bool draw(Kind &k, uint32_t columns, uint32_t rows, const xrit_geo_nav *nav, const xrit_geo_grid *grid)
    {
        k.key.clear();
        k.pitch = (columns + 3) & ~3u;
        mask.assign((size_t)k.pitch * rows, 0);
        for (int layer = 0; layer < 2; ++layer) {
            const size_t n = lon[layer].size();
            points.resize(n);
            if (nav) {
                quads.resize(4 * n);
                if (xrit_overlay_quads(lon[layer].data(), lat[layer].data(), n, nav->sub_lon_deg, quads.data()) != XRIT_OK ||
                    xrit_overlay_map(k.ov, nav, quads.data(), n, points.data()) != XRIT_OK)
                    return fail("overlay map");
            } else if (xrit_overlay_grid_points(grid, lon[layer].data(), lat[layer].data(), n, points.data()) != XRIT_OK) {
                return fail("overlay grid points");
            }
            // (a layer without vertices is drawn too: the last draw is the one that leaves the mask on the device)
            xrit_overlay_draw_summary sum{};
            if (xrit_overlay_draw(k.ov, points.data(), n, (uint32_t)layer, width, nav ? 0u : columns * 128u, mask.data(), columns, rows, k.pitch, 0,
                                  &sum) != XRIT_OK)
                return fail("overlay draw");
        }
        ++drawn;
        return true;
    }
    // d_view: a toned view (8 bits, tight) in device memory; path: it with the map, as binary PPM
    bool write(const std::string &path, const uint8_t *d_view, uint32_t columns, uint32_t rows, const xrit_geo_nav *nav, const xrit_geo_grid *grid)
    {
        Kind &k = kinds[nav ? 0 : 1];
        char text[256];
        if (nav)
            std::snprintf(text, sizeof text, "%u %u %d %d %d %d %d %.17g", columns, rows, nav->cfac, nav->lfac, nav->coff, nav->loff, nav->origin,
                          nav->sub_lon_deg);
        else
            std::snprintf(text, sizeof text, "%u %u %u %.17g %.17g %.17g %.17g", columns, rows, grid->kind, grid->lon0_deg, grid->lat0_deg,
                          grid->step_lon_deg, grid->step_lat_deg);
        if (k.key != text) {
            if (!draw(k, columns, rows, nav, grid)) return false;
            k.key = text;
        }
        const uint8_t *d_mask = nullptr;
        if (xrit_overlay_mask_device(k.ov, &d_mask) != XRIT_OK || !d_mask) return fail("overlay mask");
        const xrit_product_image image{d_view, columns, rows, columns, 8};
        out.resize((size_t)columns * rows * 3);
        xrit_overlay_blend_summary blended{};
        if (xrit_overlay_blend_resident(k.ov, &image, 1, d_mask, k.pitch, styles, out.data(), columns * 3, 3, &blended) != XRIT_OK)
            return fail("overlay blend");
        if (!write_pnm(path, out.data(), 3, columns, rows)) return false;
        ++written;
        return true;
    }
    void report() const { std::fprintf(stderr, "overlay: %zu views written with the map (%zu masks drawn), %zu skipped\n", written, drawn, skipped); }
};

// ---- the sequence ------------------------------------------------------------------------------------------------------
struct DecodeChain {
    bool hrit = false, decompress = false;
    int device = 0;
    Rows rows;
    Windows windows;
    Framer framer;
    Lock lock;
    Decoder decoder;
    Demux demux;
    Packets packets;
    Files files;
    Images images;
    Canvas canvas;          // (declared before the three that work on its pixels: they are released first)
    Products products;
    Jpeg jpeg;
    Projection projection;
    MapOverlay overlay;
    JpegFiles jpeg_files;

    bool active() const { return decoder.dec || lock.lk; }

    // every stage the options ask for, in the order of the data; false (after a line on stderr) at the first that does not open
    bool open(const Options &o)
    {
        hrit = o.mode == "hrit";
        device = o.device;
        if (o.flywheel) {
            if (xrit_lock_create(&lock.lk.p, hrit ? 1 : 0, device) != XRIT_OK || xrit_lock_set_flywheel(lock.lk, (uint32_t)o.flywheel) != XRIT_OK)
                return library_error();
        } else if (xrit_decoder_create(&decoder.dec.p, hrit ? 1 : 0, device) != XRIT_OK) {
            return library_error();
        }
        if (o.stream_sync && !o.flywheel && xrit_framer_create(&framer.fr.p, hrit ? 1 : 0, device) != XRIT_OK) return library_error();
        if (!o.decode.empty() && !decoder.out.open(o.decode, "decode output")) return false;
        if (o.channels.empty() && o.decoder_stats.empty() && o.packets.empty() && o.files.empty()) return true;
        if (xrit_demux_create(&demux.dm.p, device) != XRIT_OK || xrit_demux_stats(demux.dm, &demux.stats) != XRIT_OK) return library_error();
        if (!o.channels.empty() && !make_dir(o.channels, "--channels")) return false;
        demux.channel_dir = o.channels;
        if (!o.decoder_stats.empty() && !demux.stats_out.open(o.decoder_stats, "decoder statistics output")) return false;
        if (o.packets.empty() && o.files.empty()) return true;
        if (xrit_packets_create(&packets.pk.p, device) != XRIT_OK) return library_error();
        if (!o.packets.empty() && !make_dir(o.packets, "--packets")) return false;
        packets.dir = o.packets;
        if (o.files.empty()) return true;
        if (xrit_files_create(&files.fa.p, device) != XRIT_OK) return library_error();
        if (!make_dir(o.files, "--files")) return false;
        files.dir = o.files;
        if (o.files_jpeg.on && xrit_jpegdec_create(&jpeg_files.jd.p, device) != XRIT_OK) return library_error();
        decompress = o.files_decompress;
        if (!decompress) return true;
        if (xrit_images_create(&images.im.p, device) != XRIT_OK) return library_error();
        if (!o.canvas) return true;
        canvas.n_slots = o.canvas_slots;
        if (xrit_canvas_create(&canvas.cv.p, device, canvas.n_slots, o.canvas_mib << 20) != XRIT_OK) return library_error();
        canvas.slots.assign(canvas.n_slots, xrit_canvas_slot{});
        canvas.pixels.resize(o.canvas_mib << 20);
        products.params = o.product;
        if (o.products && xrit_product_create(&products.pr.p, device) != XRIT_OK) return library_error();
        jpeg.quality = o.jpeg;
        if (o.products && o.jpeg && xrit_jpeg_create(&jpeg.jp.p, device) != XRIT_OK) return library_error();
        projection.grid = o.project_grid;
        projection.grid_given = o.project_grid_given;
        projection.mode = o.project_mode;
        if (o.project && xrit_geo_create(&projection.geo.p, device) != XRIT_OK) return library_error();
        projection.nav.assign(canvas.n_slots, Projection::SlotNav{});
        if (o.overlay.on() && !overlay.open(device)) return library_error();
        return !overlay.on() || overlay.load(o.overlay);
    }
    // a call's quantised symbols: the frames found in them, decoded, and through every stage behind
    bool add(const int8_t *sym, size_t n)
    {
        size_t take = 0;
        if (lock.lk) {
            if (!lock.find(rows, sym, n, take)) return false;
        } else {
            if (!(framer.fr ? framer.find(rows, sym, n, take) : windows.find(rows, sym, n, hrit, device, take))) return false;
            if (take && !decoder.decode(rows, take)) return false;
        }
        if (take == 0) return true;
        if (!decoder.account(rows, take)) return false;
        if (!demux.dm) return true;
        if (!demux.process(rows, take)) return false;
        if (!packets.pk) return true;
        if (!packets.process(demux)) return false;
        if (!files.fa) return true;
        if (!files.process(packets)) return false;
        if (images.im && !images.process(files)) return false;
        if (canvas.cv && !place_lines()) return false;
        return journal();
    }
    // every record's bytes appended to its file, which is renamed at its end and deleted when it is aborted; here what is
    // open waits as the .part file
    bool journal()
    {
        for (size_t i = 0; i < files.summary.files; ++i) {
            const xrit_file_record &r = files.recs[i];
            const Span body{files.bytes.data() + r.offset, r.length};
            // the image stage's verdict: a rice-coded image's record (begun in this round, or open since an earlier one)
            const bool rice = images.im && images.files[i].rice;
            const std::vector<Span> none, &lines = rice ? images.lines_of(i) : none;
            if (!journal_record(file_stem(files.dir, r.vcid, r.apid, r.key_serial), r.flags, r.n_pieces ? &body : nullptr, rice, lines.data(),
                                lines.size()))
                return false;
            if (jpeg_files.jd && r.compression == 2 && (r.flags & XRIT_FILE_ENDS) && !(r.flags & XRIT_FILE_ABORTED) &&
                !jpeg_files.write(file_stem(files.dir, r.vcid, r.apid, r.key_serial), r))
                return false;
        }
        return true;
    }
    // the canvases that became complete are read, written and released
    bool place_lines()
    {
        if (!canvas.process(files, images)) return false;
        if (projection.geo || overlay.on()) projection.note_navigation(files, canvas);
        for (unsigned s = 0; canvas.summary.completed && s < canvas.n_slots; ++s) {
            if (!canvas.slots[s].in_use || !canvas.slots[s].complete) continue;
            if (!write_canvas(s, false)) return false;
            if (xrit_canvas_release(canvas.cv, s) != XRIT_OK) return fail("canvas release");
            canvas.slots[s] = xrit_canvas_slot{};
            projection.nav[s] = Projection::SlotNav{};
        }
        return true;
    }
    // one canvas as binary PGM, and what --products and --project make of it
    bool write_canvas(unsigned s, bool partial)
    {
        xrit_canvas_slot info{};
        if (xrit_canvas_read(canvas.cv, s, canvas.pixels.data(), canvas.pixels.size(), &info) != XRIT_OK) return fail("canvas read");
        const std::string stem = files.dir + "/" + canvas_name(info.name, sizeof info.name, info.vcid, info.image_id, info.born_call) +
                                 (partial ? ".partial" : "");
        if (!write_pgm(stem + ".pgm", canvas.pixels.data(), info.max_column, info.max_row, info.pitch, info.bits)) return false;
        ++canvas.written;
        if (products.pr && !products.write(canvas, s, info, stem, jpeg)) return false;
        if (overlay.on() && info.max_column && info.max_row) {          // the toned view lies where the product call left it
            const Projection::SlotNav &n = projection.nav[s];
            if (n.state == 1) {
                if (!overlay.write(stem + ".view.map.ppm", product_view(), info.max_column, info.max_row, &n.nav, nullptr)) return false;
            } else {
                std::fprintf(stderr, "overlay: %s: no image navigation record of a file at line 0, column 0, no map drawn\n", stem.c_str());
                ++overlay.skipped;
            }
        }
        if (projection.geo && !projection.write(canvas, s, info, stem, products)) return false;
        if (overlay.on() && projection.geo && projection.wrote_view)
            return overlay.write(stem + ".geo.view.map.ppm", product_view(), projection.grid.columns, projection.grid.rows, nullptr, &projection.grid);
        return true;
    }
    // the toned image of the product handle's last host-buffer or resident call, on the device
    const uint8_t *product_view()
    {
        const uint8_t *d_tone = nullptr, *d_small = nullptr;
        if (xrit_product_outputs_device(products.pr, &d_tone, &d_small) != XRIT_OK) fail("product outputs");
        return d_tone;
    }
    // the end of the run: what is incomplete becomes .partial.pgm, and every open stage's line on stderr
    void close()
    {
        if (active()) decoder.report();
        if (lock.lk) lock.report();
        if (framer.fr) framer.report();
        if (demux.dm) demux.report();
        if (files.fa) files.report();
        if (files.fa && decompress) images.report();
        if (jpeg_files.jd) jpeg_files.report();
        if (canvas.cv) {
            size_t partial = 0;
            for (unsigned s = 0; s < canvas.n_slots; ++s)
                if (canvas.slots[s].in_use && write_canvas(s, true)) ++partial;
            canvas.report(partial);
            if (products.pr) products.report();
            if (jpeg.jp) jpeg.report();
            if (projection.geo) projection.report();
            if (overlay.on()) overlay.report();
        }
        if (packets.pk) packets.report();
    }
};

// ---- --monitor: the link monitor's rows as CSV, and what the run's summary needs ------------------------------------------
struct Monitor {
    Handle<xrit_monitor, xrit_monitor_destroy> mon;
    File csv;
    std::vector<xrit_monitor_block> rows;
    std::vector<double> esn0;           // esn0_m2m4_db of every block, for the median
    uint64_t symbols = 0, sat = 0;

    bool open(const std::string &path, unsigned block, int device)
    {
        if (xrit_monitor_create(&mon.p, block, XRIT_SYMBOL_F32, device) != XRIT_OK) return library_error("monitor");
        if (!csv.open(path, "monitor", "w")) return false;
        std::fprintf(csv.f, "first,n,level,dc,esn0_m2m4_db,esn0_snv_db,flip_rate,sat_rate,flags\n");
        return true;
    }
    bool add(const float *soft, size_t n)
    {
        rows.resize(xrit_monitor_rows(mon, n) + 1);
        size_t got = 0;
        if (xrit_monitor_push(mon, soft, n, rows.data(), rows.size(), &got) != XRIT_OK) return library_error("monitor");
        for (size_t i = 0; i < got; ++i) {
            xrit_monitor_quality q;
            if (xrit_monitor_derive(&rows[i], XRIT_SYMBOL_F32, &q) != XRIT_OK) return library_error("monitor");
            std::fprintf(csv.f, "%llu,%u,%.6f,%.6f,%.3f,%.3f,%.6f,%.6f,%u\n", (unsigned long long)rows[i].first, rows[i].n, q.level, q.dc,
                         q.esn0_m2m4_db, q.esn0_snv_db, q.flip_rate, q.sat_rate, q.flags);
            esn0.push_back(q.esn0_m2m4_db);
            symbols += rows[i].n;
            sat += rows[i].sat;
        }
        return true;
    }
    // the median over the run (the upper of the two middle blocks), the blocks more than 3 dB under it, the sink's saturation
    void report() const
    {
        if (!mon || !csv.f) return;
        if (esn0.empty()) {
            std::fprintf(stderr, "monitor: no block completed\n");
            return;
        }
        std::vector<double> sorted(esn0);
        std::sort(sorted.begin(), sorted.end());
        const double median = sorted[sorted.size() / 2];
        size_t low = 0;
        for (double v : esn0) low += v < median - 3.0;
        std::fprintf(stderr, "monitor: %zu blocks, median Es/N0 %.2f dB, %zu blocks more than 3 dB under it, %.4f %% of the symbols saturate int8\n",
                     esn0.size(), median, low, 100.0 * (double)sat / (double)symbols);
    }
};
