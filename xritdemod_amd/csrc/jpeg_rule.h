// jpeg_rule.h -- the JPEG stage's rules per value, one set of functions for the kernels (jpeg.hip), the host parts
// (jpeg.cpp: the header, the bound) and the stand-alone check (jpeg_host_check.cpp, make jpeg-host-check): the 1-D pass of
// the slow-integer forward DCT (jfdctint: 13-bit constants, PASS1_BITS 2), libjpeg's quantiser, its 16-bit fixed-point
// RGB -> YCbCr, category and magnitude bits, the quality scaling, and the Annex K Huffman tables as code / length per
// symbol.  tests/jpeg_spec.py is the specification; every function here equals it value for value.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

namespace xrit {

constexpr uint32_t JPEG_MAX_DIM = 65535;
constexpr uint32_t JPEG_MAX_BLOCKS = 1u << 22;          // 8 x 8 blocks of all components that one call takes
constexpr uint32_t JPEG_BLOCK_BITS = 22 + 63 * 26;      // the longest block: DC 11 + 11 bits (chrominance), 63 x (16-bit code + 10 bits)
constexpr uint32_t JPEG_MAX_HEADER = 640;               // SOI .. SOS of three components with DRI: 623 bytes

// zigzag position k -> natural index (row * 8 + column)
constexpr uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1, natural order
constexpr uint8_t JPEG_STD_LUMINANCE[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                            69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                            81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t JPEG_STD_CHROMINANCE[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: the number of codes of each length 1 .. 16, then the symbols in code order.  Tables 0 .. 3 in the order
// libjpeg writes them for a colour scan: DC luminance, AC luminance, DC chrominance, AC chrominance.
struct JpegHuffSpec {
    uint8_t cls, index;
    uint8_t bits[16];
    uint16_t count;
    uint8_t vals[162];
};
constexpr JpegHuffSpec JPEG_HUFF_SPEC[4] = {
    {0, 0, {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {1, 0, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}},
    {0, 1, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {1, 1, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}},
};

// symbol -> code << 8 | length (0: no such symbol), by Annex C
struct JpegCodes {
    uint32_t e[256];
};
constexpr JpegCodes jpeg_make_codes(const JpegHuffSpec &s)
{
    JpegCodes t{};
    uint32_t code = 0, k = 0;
    for (uint32_t length = 1; length <= 16; ++length) {
        for (uint32_t i = 0; i < s.bits[length - 1]; ++i) t.e[s.vals[k++]] = code++ << 8 | length;
        code <<= 1;
    }
    return t;
}
struct JpegCodeTables {
    JpegCodes t[4];
};
constexpr JpegCodeTables jpeg_make_code_tables()
{
    return {{jpeg_make_codes(JPEG_HUFF_SPEC[0]), jpeg_make_codes(JPEG_HUFF_SPEC[1]), jpeg_make_codes(JPEG_HUFF_SPEC[2]),
             jpeg_make_codes(JPEG_HUFF_SPEC[3])}};
}

JPEG_HD int32_t jpeg_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of jfdctint over d[0 .. 8), in place; second: the column pass's scaling.  The products fit 32 bits: the
// row pass takes |d| <= 128, the column pass its outputs (|.| < 5800).
JPEG_HD void jpeg_dct_pass(int32_t *d, bool second)
{
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = second ? 15 : 11;
    d[0] = second ? jpeg_descale(t10 + t11, 2) : (t10 + t11) * 4;
    d[4] = second ? jpeg_descale(t10 - t11, 2) : (t10 - t11) * 4;
    const int32_t y1 = (t12 + t13) * 4433;
    d[2] = jpeg_descale(y1 + t13 * 6270, n);
    d[6] = jpeg_descale(y1 - t12 * 15137, n);
    const int32_t z5 = (t4 + t6 + t5 + t7) * 9633;
    const int32_t z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d[7] = jpeg_descale(t4 * 2446 + z1 + z3, n);
    d[5] = jpeg_descale(t5 * 16819 + z2 + z4, n);
    d[3] = jpeg_descale(t6 * 25172 + z2 + z3, n);
    d[1] = jpeg_descale(t7 * 12299 + z1 + z4, n);
}

// libjpeg's quantiser on the transform's output (scaled by 8): divisor q << 3, halves away from zero
JPEG_HD int32_t jpeg_quantise(int32_t c, uint32_t q)
{
    const uint32_t qv = q << 3, a = (uint32_t)(c < 0 ? -c : c), m = (a + (qv >> 1)) / qv;
    return c < 0 ? -(int32_t)m : (int32_t)m;
}

// libjpeg's rgb_ycc_convert: 16-bit fixed point
JPEG_HD void jpeg_colour(int32_t r, int32_t g, int32_t b, int32_t &y, int32_t &cb, int32_t &cr)
{
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the number of bits of |v| (the category), and the magnitude bits: v, or v - 1 for a negative v, in that many bits
JPEG_HD uint32_t jpeg_category(int32_t v, uint32_t &bits)
{
    uint32_t a = (uint32_t)(v < 0 ? -v : v), cat = 0;
    while (a) { ++cat; a >>= 1; }
    bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1);
    return cat;
}

// jpeg_quality_scaling and jpeg_add_quant_table with force_baseline; quality 1 .. 100
JPEG_HD uint32_t jpeg_quality_entry(uint32_t base, uint32_t quality)
{
    const uint32_t s = quality < 50 ? 5000 / quality : 200 - 2 * quality, e = (base * s + 50) / 100;
    return e < 1 ? 1 : e > 255 ? 255 : e;
}

}  // namespace xrit
