// The zig-zag order the Huffman encoder's kernels compile in (huffman_encode.hip stages every block's row in this order with
// compile-time halfword selectors).  Plain C++: tests/test_gpu_huffman_encode_pipeline.py includes it in a host-only program next to
// host::jpeg_zigzag_to_natural(), the table the library uploads, so the two cannot drift.
#ifndef UHDR_HUFF_ZIGZAG_H
#define UHDR_HUFF_ZIGZAG_H
#include <stdint.h>

namespace uhdr {

// zig-zag position -> natural index (ITU-T T.81 figure A.6)
constexpr uint8_t kHuffZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

}  // namespace uhdr
#endif
