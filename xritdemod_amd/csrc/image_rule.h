// image_rule.h -- the image stage's decision per file record and the state it leaves per key (include/xritdemod_amd.h,
// "Image lines"; tests/image_spec.py states the same), as plain integer functions for the device (images.hip) and the
// host (image_host_check.cpp holds them against a table recorded from the specification).
#pragma once

#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

constexpr uint32_t IMAGE_BEGUN = 1, IMAGE_COMPLETED = 2, IMAGE_ABORTED = 4;

struct ImageMark {
    uint32_t rice;                  // the record's pieces (behind the first with BEGINS) are Rice-coded lines
    uint32_t continued;             // ... of the image the key's state holds open
    uint32_t n_lines, first_row;
    uint32_t padded;                // bytes of one line in the output: columns * width rounded up to a multiple of 4
    uint32_t events;                // IMAGE_BEGUN | IMAGE_COMPLETED | IMAGE_ABORTED, of a rice record
    uint32_t base_lines, base_faults;   // what the image had before this call (continued) or 0
};

// bits per pixel, pixels per block and columns inside the Rice decoder's ranges
XRIT_HD inline bool image_params_ok(const xrit_file_record &r)
{
    return r.bits_per_pixel >= 1 && r.bits_per_pixel <= 16 && r.columns >= 1 &&
           (r.pixels_per_block == 8 || r.pixels_per_block == 16 || r.pixels_per_block == 32 || r.pixels_per_block == 64);
}

XRIT_HD inline uint32_t image_line_bytes(const xrit_file_record &r) { return (uint32_t)r.columns * (r.bits_per_pixel <= 8 ? 1u : 2u); }

// first_length, first_index: length and index_in_file of the record's first piece of the call (0, 0 when it has none)
XRIT_HD inline ImageMark image_mark(const xrit_file_record &r, uint32_t first_length, uint32_t first_index, const xrit_image_key &k)
{
    ImageMark m{};
    const bool begins = r.flags & XRIT_FILE_BEGINS;
    if (begins)
        m.rice = r.n_pieces >= 1 && r.header_state == 2 && r.file_type == 0 && r.compression == 1 && image_params_ok(r) &&
                 r.header_length == first_length;
    else
        m.rice = m.continued = k.open && k.key_serial == r.key_serial && image_params_ok(r);
    if (!m.rice) return m;
    m.n_lines = r.n_pieces - (begins ? 1u : 0u);
    m.base_lines = m.continued ? k.lines : 0u;
    m.base_faults = m.continued ? k.faults : 0u;
    m.first_row = begins ? 0u : (r.n_pieces ? (first_index ? first_index - 1u : 0u) : m.base_lines);
    m.padded = (image_line_bytes(r) + 3u) & ~3u;
    m.events = (begins ? IMAGE_BEGUN : 0u) | ((r.flags & XRIT_FILE_ENDS) ? IMAGE_COMPLETED : 0u) |
               ((r.flags & XRIT_FILE_ABORTED) ? IMAGE_ABORTED : 0u);
    return m;
}

// what the key carries after a call whose last record of that key is r (marked m, `faults` of its lines faulted)
XRIT_HD inline xrit_image_key image_next(const xrit_file_record &r, const ImageMark &m, uint32_t faults)
{
    xrit_image_key k{};
    k.key_serial = r.key_serial;
    if (m.rice) {
        k.open = !(r.flags & (XRIT_FILE_ENDS | XRIT_FILE_ABORTED));
        k.lines = m.base_lines + m.n_lines;
        k.faults = m.base_faults + faults;
    }
    return k;
}

}  // namespace xrit
