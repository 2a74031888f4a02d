// jpeg_files.h -- the plain parts of --files-jpeg: the option on the command line, where an assembled file's data field
// begins, and binary PNM (P5 for one component, P6 for three).  No library call: checked by `make host-program-check`.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

// the option: a switch that needs --files DIR.  flag(): true when `a` is it; refused(): why the line is refused, or nullptr
struct FilesJpegOption {
    bool on = false;
    bool flag(const std::string &a)
    {
        if (a != "--files-jpeg") return false;
        return on = true;
    }
    const char *refused(bool files_given) const { return on && !files_given ? "--files-jpeg needs --files DIR\n" : nullptr; }
};

// The file assembler strips the 10-byte transport header (file counter, length in bits) from the first packet: STEM.lrit
// begins with the primary header, and the data field lies behind the header chain, `header_length` bytes in.  A chain that
// was not walked to its end (header_state != 2) or that is longer than the file has no data field: 0, *n = 0.
inline size_t data_field(uint32_t header_length, uint32_t header_state, size_t file_bytes, size_t *n)
{
    *n = 0;
    if (header_state != 2 || header_length < 16 || header_length > file_bytes) return 0;
    *n = file_bytes - header_length;
    return header_length;
}

inline std::string pnm_header(uint32_t components, uint32_t columns, uint32_t rows)
{
    return std::string(components == 3 ? "P6\n" : "P5\n") + std::to_string(columns) + " " + std::to_string(rows) + "\n255\n";
}
inline const char *pnm_suffix(uint32_t components) { return components == 3 ? ".ppm" : ".pgm"; }

// tight rows of 8-bit samples, one or three per pixel
inline bool write_pnm(const std::string &path, const uint8_t *pixels, uint32_t components, uint32_t columns, uint32_t rows)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); return false; }
    const std::string head = pnm_header(components, columns, rows);
    const size_t n = (size_t)columns * rows * components;
    const bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size() && std::fwrite(pixels, 1, n, f) == n;
    std::fclose(f);
    if (!ok) std::perror(path.c_str());
    return ok;
}
