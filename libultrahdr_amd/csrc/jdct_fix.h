// The 13-bit fixed-point constants of libjpeg's JDCT_ISLOW transforms (jfdctint.c and jidctint.c share them: CONST_BITS 13,
// FIX(x) = round(x * 8192)).  Used by idct_core.h and fdct_core.h.
#pragma once

namespace uhdr {

constexpr int FIX_0_298631336 = 2446;
constexpr int FIX_0_390180644 = 3196;
constexpr int FIX_0_541196100 = 4433;
constexpr int FIX_0_765366865 = 6270;
constexpr int FIX_0_899976223 = 7373;
constexpr int FIX_1_175875602 = 9633;
constexpr int FIX_1_501321110 = 12299;
constexpr int FIX_1_847759065 = 15137;
constexpr int FIX_1_961570560 = 16069;
constexpr int FIX_2_053119869 = 16819;
constexpr int FIX_2_562915447 = 20995;
constexpr int FIX_3_072711026 = 25172;

}  // namespace uhdr
