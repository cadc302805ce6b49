// Host-side table builders.  The look-up tables the reference builds lazily on the CPU
// (LookUpTable, GainLUT, ShepardsIDW) are built here with the host's own libm -- the same libm the
// reference would call on this machine -- and uploaded, because device transcendental functions
// do not round identically to glibc's.  See host_tables.cpp for the per-call-site float/double
// notes.
#pragma once
#include <functional>
#include <vector>

#include "uhdr_types.h"

namespace uhdr {
namespace host {

const std::vector<float>& srgb_inv_oetf_lut();  // 1024  (gainmapmath.cpp:126-131)
const std::vector<float>& hlg_inv_oetf_lut();   // 4096  (gainmapmath.cpp:271-277)
const std::vector<float>& pq_inv_oetf_lut();    // 4096  (gainmapmath.cpp:339-345)
const std::vector<float>& hlg_inv_oetf_ootf_lut();  // 4096: hlgInvOetfLUT then hlgOotfApprox per node
const std::vector<float>& hlg_oetf_lut();       // 65536 (gainmapmath.cpp:248-254)
const std::vector<float>& pq_oetf_lut();        // 65536 (gainmapmath.cpp:320-326)
const std::vector<float>& pq_oetf_code_lut();   // 65536 uint16 codes (pqOetfLUT then colorToRgba1010102), packed two per float

// 10-bit output-code thresholds of the HLG / PQ tail (kOetfThrN floats; see host_tables.cpp)
const std::vector<float>& oetf_code_thresholds(int ct);
uint32_t oetf_code(int ct, float v);  // the composite itself, evaluated with the host libm
// the same step function as a bucket table for the quad kernel (see host_tables.cpp)
struct OetfBuckets {
  uint32_t shift = 0, base = 0, n = 0;  // bucket k covers bit patterns [(base + k) << shift, (base + k + 1) << shift)
  uint32_t lo_bits = 0, hi_bits = 0;    // the domain: the device clamps the bit pattern into it first
  uint32_t clamp_lo_bits = 0;           // max(lo_bits, base << shift): the device's lower clamp, so that bucket - base never underflows
  bool exact = false;                   // construction verified (one threshold per bucket, replay against the composite)
  std::vector<uint32_t> entries;        // n x {thr, lo | hi << 16}
};
OetfBuckets build_step_table(const std::function<uint32_t(uint32_t)>& code_of_bits, uint32_t lo_bits, uint32_t hi_bits, uint32_t shift, uint32_t capacity);
const OetfBuckets& oetf_code_buckets(int ct, bool prescaled = false);  // prescaled: argument is the value before (x * 203) / peak
// applyGainMap with gamma != 1: GainLUT::getGainFactor's table index (gainmapmath.h:483-489) as thresholds over the gain value
// (see host_tables.cpp).  One table per distinct 1 / gamma, built once per process.
struct GammaIndexTable {
  float gamma_inv = 0.0f;
  bool exact = false;          // construction verified; false: no table for this gamma, the caller keeps the pow per sample
  double build_ms = 0.0;       // host time of the construction, checks included
  // kGammaThrN floats, T[i] at thr[1 + i]: T[-1] = 0 (read, never decisive), T[0] = 0, T[i] the smallest float whose index is >= i,
  // T[1024] = T[1025] = +inf
  std::vector<float> thr;
};
uint32_t gamma_index_direct(float gain, float gamma_inv);  // the reference's expression itself, with the host libm
const GammaIndexTable& gamma_index_table(float gamma_inv);
// the device's lookup (apply_gainmap.hip: gain_index) restated on the host: an estimate from float log2 / exp2, settled and
// confirmed on two adjacent thresholds, else a binary search over T
uint32_t gamma_index_lookup(float gain, const float* T, float gamma_inv);  // T = thr.data() + 1
// generateGainMap with gamma != 1: the two byte functions of the encode side as thresholds over their float argument
//   form 0 (one pass, encodeGain gainmapmath.cpp:769-770):    (uint8_t)(powf(n, gamma) * 255.0f)
//   form 1 (two pass, affineMapGain gainmapmath.cpp:784-789): m = (float)pow((double)m, (double)gamma); clip(m * 255 + 0.5, 0, 255)
// Domains: form 1 answers for EVERY finite float m (negative -> 0, anything from T[255] on -> 255); form 0
// answers for every n of [-1e-6, kGammaCodeHi0 = four ulps past 1.0f] (negative -> 0), beyond which the reference's narrowing of a
// product >= 256 or <= -1 is not a step function any more (encodeGain's n stays within an ulp of [0, 1]).  An even-integer gamma
// maps a negative argument to the byte of its magnitude, as pow does: the sign bit of T[0] says so (host_tables.cpp).
struct GammaCodeTable {
  float gamma = 0.0f;
  bool exact = false;            // both sets verified; false: no table for this gamma, the caller keeps the pow per sample
  double build_ms = 0.0;         // host time of the construction, checks included
  std::vector<float> thr;        // 2 x kGammaCodeN: form 0's T[0..255], then form 1's; T[0] = +-0, T[k] the smallest float whose byte is >= k
  float min_gap[2] = {0, 0};     // the smallest T[k + 1] - T[k], k = 1..254, per form (the device table builder's bucket width)
  uint32_t min_gap_ulps[2] = {0, 0};  // the same distance in bit patterns
};
constexpr uint32_t kGammaCodeHi0 = 0x3f800004u;  // bit pattern of the last float of form 0's domain
uint32_t gamma_code_direct(float v, float gamma, int form);  // the reference's expression itself, with the host libm
uint32_t gamma_code_lookup(float v, const float* T);         // the device's lookup (gamma_code.h) restated: eight steps over T[0..255]
const GammaCodeTable& gamma_code_table(float gamma);
// encode side (see host_tables.cpp): toneMap's sRGB byte, encodeGain's byte, RGBA1010102 code -> linear value
const OetfBuckets& srgb_code8_buckets();
OetfBuckets gain_code8_buckets(float min_boost, float max_boost, float log2min, double log2_range, double log2_range_rcp, float gamma = 1.0f);
std::vector<float> lin10_table(const float* lut, int n);
float gain_cap_ratio();                            // computeGain's 2.3f cap in the ratio domain (0: not representable)
const std::vector<float>& srgb_inv_oetf_of_byte(); // 256: byte -> byte / 255.0f -> sRGB inverse-OETF table value

// float64 tables of exact_math.h (table-driven pow / log2 of the encode path)
const std::vector<double>& math_tables();

Yuv2Rgb yuv2rgb_coeffs(int cg);  // gainmapmath.cpp:94,104-105 / 164,174-175 / 194,226-227
Rgb2Yuv rgb2yuv_coeffs(int cg);
void luminance_coeffs(int cg, float out[3]);  // gainmapmath.cpp:86, 156, 187
// getGamutConversionFn(dst, src) (gainmapmath.cpp:1087-1129): returns false for UNSPECIFIED;
// *identity set when dst == src.
bool gamut_matrix(int dst_cg, int src_cg, Mat3* out, bool* identity);
// convertYuv coefficient choice (jpegr.cpp:436-502): 0 ok, 1 identity (nothing to do), <0 error
int yuv_encoding_matrix(int src_cg, int dst_cg, Mat3* out);

float reference_peak_nits(int ct);  // getReferenceDisplayPeakLuminanceInNits (gainmapmath.cpp:20-34)

bool metadata_channels_identical(const uhdr_gainmap_metadata_t& m);  // ultrahdrcommon.h:218-226
// gainmap_weight from the display boost (jpegr.cpp:1678-1689; log2f because jpegr.cpp has
// `using namespace std`)
float gainmap_weight(const uhdr_gainmap_metadata_t& m, float max_display_boost);
// Fills the ApplyTables block (uhdr_types.h) for one applyGainMap call.
void build_apply_tables(const uhdr_gainmap_metadata_t& m, float weight, int idw_scale,
                        std::vector<float>* out);
void fill_idw(float* w, int s, int inc_r, int inc_b);  // gainmapmath.cpp:43-80

// libjpeg quality -> quant table (jcparam.c jpeg_quality_scaling / jpeg_add_quant_table with
// force_baseline; natural order)
void jpeg_quant_table(int quality, int is_chroma, uint16_t qt[64]);

// baseline Huffman stage (T.81 Annex K.3 tables, Annex C codes)
constexpr int kHuffTabWords = 2 * (16 + 256);
const uint8_t* jpeg_zigzag_to_natural();  // 64 entries
int jpeg_std_huff_table(int is_ac, int is_chroma, uint8_t bits[17], uint8_t vals[256]);  // returns the number of symbols
const std::vector<uint32_t>& jpeg_huff_code_tables();  // kHuffTabWords packed entries (length << 16 | code)

}  // namespace host
}  // namespace uhdr
