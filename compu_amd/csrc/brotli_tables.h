// RFC 7932 constant tables of the brotli decoder (brotli.hip), in plain C++ so that host code and the tests can compile them.
// The 122 784-byte static dictionary is data (brotli_dict.bin), turned into a device array by build.sh.
#pragma once
#include <stdint.h>

#ifndef BROTLI_TAB_SPACE
#define BROTLI_TAB_SPACE  // brotli.hip defines it as __device__
#endif

namespace brotli_tab {

// Appendix B: word transforms.  Types: 0 identity, 1..9 omit the last 1..9 bytes, 10 uppercase the first character,
// 11 uppercase all, 12..20 omit the first 1..9 bytes.
enum { T_IDENTITY = 0, T_OMIT_LAST_9 = 9, T_UPPER_FIRST = 10, T_UPPER_ALL = 11, T_OMIT_FIRST_1 = 12, T_OMIT_FIRST_9 = 20 };
constexpr int NUM_TRANSFORMS = 121;
struct Transform {
    char prefix[6];
    uint8_t prefix_len;
    uint8_t type;
    char suffix[9];
    uint8_t suffix_len;
};
BROTLI_TAB_SPACE static const Transform TRANSFORMS[NUM_TRANSFORMS] = {
    {"", 0, 0, "", 0}, /*   0 */
    {"", 0, 0, " ", 1}, /*   1 */
    {" ", 1, 0, " ", 1}, /*   2 */
    {"", 0, 12, "", 0}, /*   3 */
    {"", 0, 10, " ", 1}, /*   4 */
    {"", 0, 0, " the ", 5}, /*   5 */
    {" ", 1, 0, "", 0}, /*   6 */
    {"s ", 2, 0, " ", 1}, /*   7 */
    {"", 0, 0, " of ", 4}, /*   8 */
    {"", 0, 10, "", 0}, /*   9 */
    {"", 0, 0, " and ", 5}, /*  10 */
    {"", 0, 13, "", 0}, /*  11 */
    {"", 0, 1, "", 0}, /*  12 */
    {", ", 2, 0, " ", 1}, /*  13 */
    {"", 0, 0, ", ", 2}, /*  14 */
    {" ", 1, 10, " ", 1}, /*  15 */
    {"", 0, 0, " in ", 4}, /*  16 */
    {"", 0, 0, " to ", 4}, /*  17 */
    {"e ", 2, 0, " ", 1}, /*  18 */
    {"", 0, 0, "\"", 1}, /*  19 */
    {"", 0, 0, ".", 1}, /*  20 */
    {"", 0, 0, "\">", 2}, /*  21 */
    {"", 0, 0, "\n", 1}, /*  22 */
    {"", 0, 3, "", 0}, /*  23 */
    {"", 0, 0, "]", 1}, /*  24 */
    {"", 0, 0, " for ", 5}, /*  25 */
    {"", 0, 14, "", 0}, /*  26 */
    {"", 0, 2, "", 0}, /*  27 */
    {"", 0, 0, " a ", 3}, /*  28 */
    {"", 0, 0, " that ", 6}, /*  29 */
    {" ", 1, 10, "", 0}, /*  30 */
    {"", 0, 0, ". ", 2}, /*  31 */
    {".", 1, 0, "", 0}, /*  32 */
    {" ", 1, 0, ", ", 2}, /*  33 */
    {"", 0, 15, "", 0}, /*  34 */
    {"", 0, 0, " with ", 6}, /*  35 */
    {"", 0, 0, "'", 1}, /*  36 */
    {"", 0, 0, " from ", 6}, /*  37 */
    {"", 0, 0, " by ", 4}, /*  38 */
    {"", 0, 16, "", 0}, /*  39 */
    {"", 0, 17, "", 0}, /*  40 */
    {" the ", 5, 0, "", 0}, /*  41 */
    {"", 0, 4, "", 0}, /*  42 */
    {"", 0, 0, ". The ", 6}, /*  43 */
    {"", 0, 11, "", 0}, /*  44 */
    {"", 0, 0, " on ", 4}, /*  45 */
    {"", 0, 0, " as ", 4}, /*  46 */
    {"", 0, 0, " is ", 4}, /*  47 */
    {"", 0, 7, "", 0}, /*  48 */
    {"", 0, 1, "ing ", 4}, /*  49 */
    {"", 0, 0, "\n\t", 2}, /*  50 */
    {"", 0, 0, ":", 1}, /*  51 */
    {" ", 1, 0, ". ", 2}, /*  52 */
    {"", 0, 0, "ed ", 3}, /*  53 */
    {"", 0, 20, "", 0}, /*  54 */
    {"", 0, 18, "", 0}, /*  55 */
    {"", 0, 6, "", 0}, /*  56 */
    {"", 0, 0, "(", 1}, /*  57 */
    {"", 0, 10, ", ", 2}, /*  58 */
    {"", 0, 8, "", 0}, /*  59 */
    {"", 0, 0, " at ", 4}, /*  60 */
    {"", 0, 0, "ly ", 3}, /*  61 */
    {" the ", 5, 0, " of ", 4}, /*  62 */
    {"", 0, 5, "", 0}, /*  63 */
    {"", 0, 9, "", 0}, /*  64 */
    {" ", 1, 10, ", ", 2}, /*  65 */
    {"", 0, 10, "\"", 1}, /*  66 */
    {".", 1, 0, "(", 1}, /*  67 */
    {"", 0, 11, " ", 1}, /*  68 */
    {"", 0, 10, "\">", 2}, /*  69 */
    {"", 0, 0, "=\"", 2}, /*  70 */
    {" ", 1, 0, ".", 1}, /*  71 */
    {".com/", 5, 0, "", 0}, /*  72 */
    {" the ", 5, 0, " of the ", 8}, /*  73 */
    {"", 0, 10, "'", 1}, /*  74 */
    {"", 0, 0, ". This ", 7}, /*  75 */
    {"", 0, 0, ",", 1}, /*  76 */
    {".", 1, 0, " ", 1}, /*  77 */
    {"", 0, 10, "(", 1}, /*  78 */
    {"", 0, 10, ".", 1}, /*  79 */
    {"", 0, 0, " not ", 5}, /*  80 */
    {" ", 1, 0, "=\"", 2}, /*  81 */
    {"", 0, 0, "er ", 3}, /*  82 */
    {" ", 1, 11, " ", 1}, /*  83 */
    {"", 0, 0, "al ", 3}, /*  84 */
    {" ", 1, 11, "", 0}, /*  85 */
    {"", 0, 0, "='", 2}, /*  86 */
    {"", 0, 11, "\"", 1}, /*  87 */
    {"", 0, 10, ". ", 2}, /*  88 */
    {" ", 1, 0, "(", 1}, /*  89 */
    {"", 0, 0, "ful ", 4}, /*  90 */
    {" ", 1, 10, ". ", 2}, /*  91 */
    {"", 0, 0, "ive ", 4}, /*  92 */
    {"", 0, 0, "less ", 5}, /*  93 */
    {"", 0, 11, "'", 1}, /*  94 */
    {"", 0, 0, "est ", 4}, /*  95 */
    {" ", 1, 10, ".", 1}, /*  96 */
    {"", 0, 11, "\">", 2}, /*  97 */
    {" ", 1, 0, "='", 2}, /*  98 */
    {"", 0, 10, ",", 1}, /*  99 */
    {"", 0, 0, "ize ", 4}, /* 100 */
    {"", 0, 11, ".", 1}, /* 101 */
    {"\xc2\xa0", 2, 0, "", 0}, /* 102 */
    {" ", 1, 0, ",", 1}, /* 103 */
    {"", 0, 10, "=\"", 2}, /* 104 */
    {"", 0, 11, "=\"", 2}, /* 105 */
    {"", 0, 0, "ous ", 4}, /* 106 */
    {"", 0, 11, ", ", 2}, /* 107 */
    {"", 0, 10, "='", 2}, /* 108 */
    {" ", 1, 10, ",", 1}, /* 109 */
    {" ", 1, 11, "=\"", 2}, /* 110 */
    {" ", 1, 11, ", ", 2}, /* 111 */
    {"", 0, 11, ",", 1}, /* 112 */
    {"", 0, 11, "(", 1}, /* 113 */
    {"", 0, 11, ". ", 2}, /* 114 */
    {" ", 1, 11, ".", 1}, /* 115 */
    {"", 0, 11, "='", 2}, /* 116 */
    {" ", 1, 11, ". ", 2}, /* 117 */
    {" ", 1, 10, "=\"", 2}, /* 118 */
    {" ", 1, 11, "='", 2}, /* 119 */
    {" ", 1, 10, "='", 2}, /* 120 */
};

// Section 4: dictionary words of length 4..24 -- NDBITS per length and the offset of the first word of that length.
BROTLI_TAB_SPACE static const uint8_t DICT_NDBITS[25] = {0, 0, 0, 0, 10, 10, 11, 11, 10, 10, 10, 10, 10, 9, 9, 8, 7, 7, 8, 7, 7, 6, 6, 5, 5};
BROTLI_TAB_SPACE static const uint32_t DICT_OFFSET[25] = {0, 0, 0, 0, 0, 4096, 9216, 21504, 35840, 44032, 53248, 63488, 74752,
                                                          87040, 93696, 100864, 104704, 106752, 108928, 113536, 115968, 118528,
                                                          119872, 121280, 122016};
constexpr uint32_t DICT_SIZE = 122784;

// Section 6: block count codes 0..25 -> (first length, extra bits)
BROTLI_TAB_SPACE static const uint16_t BLOCK_LEN_BASE[26] = {1, 5, 9, 13, 17, 25, 33, 41, 49, 65, 81, 97, 113, 145, 177, 209, 241, 305,
                                                             369, 497, 753, 1265, 2289, 4337, 8433, 16625};
BROTLI_TAB_SPACE static const uint8_t BLOCK_LEN_EXTRA[26] = {2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 24};

// Section 5: insert length codes 0..23 and copy length codes 0..23 -> (base, extra bits)
BROTLI_TAB_SPACE static const uint32_t INSERT_BASE[24] = {0, 1, 2, 3, 4, 5, 6, 8, 10, 14, 18, 26, 34, 50, 66, 98, 130, 194, 322, 578, 1090,
                                                          2114, 6210, 22594};
BROTLI_TAB_SPACE static const uint8_t INSERT_EXTRA[24] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24};
BROTLI_TAB_SPACE static const uint32_t COPY_BASE[24] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 18, 22, 30, 38, 54, 70, 102, 134, 198, 326, 582,
                                                        1094, 2118};
BROTLI_TAB_SPACE static const uint8_t COPY_EXTRA[24] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24};
// insert-and-copy code >> 6 -> first insert code, first copy code (Section 5, the 11 cells of the table)
BROTLI_TAB_SPACE static const uint8_t CMD_INSERT_CELL[11] = {0, 0, 0, 0, 8, 8, 0, 16, 8, 16, 16};
BROTLI_TAB_SPACE static const uint8_t CMD_COPY_CELL[11] = {0, 8, 0, 8, 0, 8, 16, 0, 16, 8, 16};

// Section 3.5: order of the code length code lengths
BROTLI_TAB_SPACE static const uint8_t CL_ORDER[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// Section 7.1: context lookup.  Row mode * 512 + p1 plus row mode * 512 + 256 + p2 (modes LSB6, MSB6, UTF8, Signed) give the
// context id of a literal from the two bytes in front of it.
struct ContextLut {
    uint8_t v[2048];
};
constexpr uint8_t utf8_p1(int c)
{
    // 0x00..0x7f of Lut0, then continuation bytes 0/1 and lead bytes 2/3 alternating
    constexpr uint8_t lo[128] = {
        0,  0,  0,  0,  0,  0,  0,  0,  0,  4,  4,  0,  0,  4,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,
        8,  12, 16, 12, 12, 20, 12, 16, 24, 28, 12, 12, 32, 12, 36, 12, 44, 44, 44, 44, 44, 44, 44, 44, 44, 44, 32, 32, 24, 40, 28, 12,
        12, 48, 52, 52, 52, 48, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 48, 52, 52, 52, 52, 52, 24, 12, 28, 12, 12,
        12, 56, 60, 60, 60, 56, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 56, 60, 60, 60, 60, 60, 24, 12, 28, 12, 0};
    return c < 128 ? lo[c] : (uint8_t)((c & 1) | (c >= 0xc0 ? 2 : 0));
}
constexpr uint8_t utf8_p2(int c)
{
    // Lut1: 0 control and space, 1 punctuation, 2 digits and upper case, 3 lower case; 0 for 0x80..0xdf, 2 for 0xe0..0xff
    return c <= 0x20 ? 0
           : c < 0x80 ? (c == 0x7f                                ? 0
                         : (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') ? 2
                         : (c >= 'a' && c <= 'z')                  ? 3
                                                                   : 1)
           : c < 0xe0 ? 0
                      : 2;
}
constexpr uint8_t signed_bucket(int c)
{
    // Lut2: 0 | 1..15 | 16..63 | 64..127 | 128..191 | 192..239 | 240..254 | 255
    return c == 0 ? 0 : c < 16 ? 1 : c < 64 ? 2 : c < 128 ? 3 : c < 192 ? 4 : c < 240 ? 5 : c < 255 ? 6 : 7;
}
constexpr ContextLut make_context_lut()
{
    ContextLut t{};
    for (int c = 0; c < 256; c++) {
        t.v[c] = (uint8_t)(c & 0x3f);            // LSB6
        t.v[256 + c] = 0;
        t.v[512 + c] = (uint8_t)(c >> 2);        // MSB6
        t.v[768 + c] = 0;
        t.v[1024 + c] = utf8_p1(c);              // UTF8
        t.v[1280 + c] = utf8_p2(c);
        t.v[1536 + c] = (uint8_t)(signed_bucket(c) << 3);  // Signed
        t.v[1792 + c] = signed_bucket(c);
    }
    return t;
}
BROTLI_TAB_SPACE static const ContextLut CONTEXT_LUT = make_context_lut();

}  // namespace brotli_tab
