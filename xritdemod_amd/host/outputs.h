// outputs.h -- the files the decode chain leaves behind, as plain file logic: binary PGM, a canvas's file name, the
// per-channel append, the packet files with their bound on open files, and the journal of a file record (.part files
// that are renamed at the record's end and removed when it is aborted).  No library call (the header is included for the
// record flags only): checked by `make host-program-check`.  Every function says what failed with perror and returns false.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/xritdemod_amd.h"

struct Span {
    const uint8_t *bytes;
    size_t length;
};

// a file that stays open over the run and is closed by scope; open() says `what` did not open
struct File {
    FILE *f = nullptr;
    File() = default;
    File(const File &) = delete;
    File &operator=(const File &) = delete;
    ~File() { if (f) std::fclose(f); }
    bool open(const std::string &path, const char *what, const char *mode = "wb")
    {
        f = std::fopen(path.c_str(), mode);
        if (!f) std::perror(what);
        return f != nullptr;
    }
};

// binary PGM: rows of `columns` samples `pitch` bytes apart (pitch = columns * width: tight rows); above 8 bits the samples
// come little-endian and go out 16-bit with the high byte first
inline bool write_pgm(const std::string &path, const uint8_t *pixels, uint32_t columns, uint32_t rows, size_t pitch, uint32_t bits)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); return false; }
    const size_t width = bits <= 8 ? 1 : 2, row_bytes = (size_t)columns * width;
    bool ok = std::fprintf(f, "P5\n%u %u\n%u\n", columns, rows, (1u << bits) - 1u) > 0;
    std::vector<uint8_t> swapped(width == 2 ? row_bytes : 0);
    for (size_t r = 0; ok && r < rows; ++r) {
        const uint8_t *src = pixels + r * pitch;
        if (width == 2) {
            for (size_t i = 0; i < row_bytes; i += 2) { swapped[i] = src[i + 1]; swapped[i + 1] = src[i]; }
            src = swapped.data();
        }
        ok = std::fwrite(src, 1, row_bytes, f) == row_bytes;
    }
    std::fclose(f);
    if (!ok) std::perror(path.c_str());
    return ok;
}

inline bool write_file(const std::string &path, const char *mode, const uint8_t *bytes, size_t length)
{
    FILE *f = std::fopen(path.c_str(), mode);
    const bool ok = f && std::fwrite(bytes, 1, length, f) == length;
    if (f) std::fclose(f);
    if (!ok) std::perror(path.c_str());
    return ok;
}

// a canvas's file name: the annotation text (up to its first NUL) reduced to [A-Za-z0-9._-], or vc<vcid>_img<image_id>_<born_call>
inline std::string canvas_name(const uint8_t *text, size_t cap, unsigned vcid, unsigned image_id, unsigned long long born_call)
{
    std::string name;
    for (size_t i = 0; i < cap && text[i]; ++i) {
        const char c = (char)text[i];
        name += (std::isalnum((unsigned char)c) || c == '.' || c == '_' || c == '-') ? c : '_';
    }
    if (name.empty()) name = "vc" + std::to_string(vcid) + "_img" + std::to_string(image_id) + "_" + std::to_string(born_call);
    return name;
}

// ChannelWriter::writeChannel: a channel's VCDUs of one round appended to DIR/channel_{vcid}.bin
inline bool append_channel(const std::string &dir, int vcid, const uint8_t *bytes, size_t length)
{
    return write_file(dir + "/channel_" + std::to_string(vcid) + ".bin", "ab", bytes, length);
}

// DIR/vc{vcid}_apid{apid}.bin: every packet whose CRC matches appended whole.  The files stay open from packet to packet,
// 64 of them at the most: a 65th key closes them all, and they are reopened for append as their packets come.
struct PacketFiles {
    static constexpr size_t MAX_OPEN = 64;
    std::map<std::pair<int, int>, FILE *> files;

    PacketFiles() = default;
    PacketFiles(const PacketFiles &) = delete;
    PacketFiles &operator=(const PacketFiles &) = delete;
    ~PacketFiles() { close(); }

    bool add(const std::string &dir, const xrit_packet &d, const uint8_t *round_bytes)
    {
        if (!d.crc_ok) return true;
        const std::pair<int, int> key{d.vcid, d.apid};
        if (files.size() >= MAX_OPEN && !files.count(key)) close();
        FILE *&f = files[key];
        const std::string name = dir + "/vc" + std::to_string(d.vcid) + "_apid" + std::to_string(d.apid) + ".bin";
        if (!f) f = std::fopen(name.c_str(), "ab");
        if (!f || std::fwrite(round_bytes + d.offset, 1, d.length, f) != d.length) { std::perror(name.c_str()); return false; }
        return true;
    }
    void close()
    {
        for (auto &kv : files)
            if (kv.second) std::fclose(kv.second);
        files.clear();
    }
};

inline std::string file_stem(const std::string &dir, unsigned vcid, unsigned apid, unsigned long long serial)
{
    return dir + "/vc" + std::to_string(vcid) + "_apid" + std::to_string(apid) + "_" + std::to_string(serial);
}

// One record of one round in the journal of its file.  `flags` are the record's (XRIT_FILE_*).  `body`, when there is one
// (the record has pieces in this round), goes to STEM.lrit.part: begun with "wb" in the round the file begins, appended
// after.  `rice` is the image stage's verdict: STEM.img.part is begun likewise, and `lines` (this round's decoded lines,
// possibly none) are appended back to back.  ENDS renames both to STEM.lrit / STEM.img, ABORTED removes them; a file that
// does neither stays .part.
inline bool journal_record(const std::string &stem, uint32_t flags, const Span *body, bool rice, const Span *lines, size_t n_lines)
{
    const std::string part = stem + ".lrit.part", img_part = stem + ".img.part";
    const bool begins = flags & XRIT_FILE_BEGINS;
    if (body && !write_file(part, begins ? "wb" : "ab", body->bytes, body->length)) return false;
    if (rice && begins && !write_file(img_part, "wb", (const uint8_t *)"", 0)) return false;
    if (rice && n_lines) {
        FILE *f = std::fopen(img_part.c_str(), "ab");
        bool ok = f != nullptr;
        for (size_t k = 0; ok && k < n_lines; ++k) ok = std::fwrite(lines[k].bytes, 1, lines[k].length, f) == lines[k].length;
        if (f) std::fclose(f);
        if (!ok) { std::perror(img_part.c_str()); return false; }
    }
    if (flags & XRIT_FILE_ABORTED) {
        std::remove(part.c_str());
        if (rice) std::remove(img_part.c_str());
    } else if (flags & XRIT_FILE_ENDS) {
        if (std::rename(part.c_str(), (stem + ".lrit").c_str()) != 0) { std::perror(part.c_str()); return false; }
        if (rice && std::rename(img_part.c_str(), (stem + ".img").c_str()) != 0) { std::perror(img_part.c_str()); return false; }
    }
    return true;
}
