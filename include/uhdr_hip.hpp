// C++ host-side mirror of ultrahdr::UltraHdr's stage operators over the C ABI of uhdr_hip.h.
//
// The reference is C++ (lib/include/ultrahdr/ultrahdrcommon.h:448-546 declares the class whose four
// methods are the hot path).  This header gives a C++ caller the same class shape -- same
// constructor knobs in the same order, same method names, argument order and error convention
// (uhdr_error_info_t by value, nothing throws) -- with the MI355X library behind it, so code written
// against ultrahdr::UltraHdr moves over by changing the type name.  Header only; link -luhdr_hip.
//
// Differences, all forced by the boundary:
//   * the first constructor argument is the device ordinal (the reference passes its GLES context there);
//   * the metadata type is the C struct uhdr_gainmap_metadata_t (uhdr_gainmap_metadata_ext_t only adds
//     the std::string version, always "1.0", ultrahdrcommon.h:446);
//   * generateGainMap returns the map in a uhdr_hip::raw_image_ext, which allocates exactly as the
//     reference's uhdr_raw_image_ext_t does (one block, stride aligned to 64 pixels,
//     lib/src/ultrahdr_api.cpp:55-117).
#pragma once
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "uhdr_hip.h"

namespace uhdr_hip {

// Owning raw image for the packed / single-plane formats a gain map uses.
struct raw_image_ext : uhdr_raw_image_t {
  raw_image_ext(uhdr_img_fmt_t fmt_, uhdr_color_gamut_t cg_, uhdr_color_transfer_t ct_, uhdr_color_range_t range_,
                unsigned w_, unsigned h_, unsigned align_stride_to) {
    std::memset(static_cast<uhdr_raw_image_t*>(this), 0, sizeof(uhdr_raw_image_t));
    fmt = fmt_; cg = cg_; ct = ct_; range = range_; w = w_; h = h_;
    const unsigned aligned_w = ((w_ + align_stride_to - 1) / align_stride_to) * align_stride_to;
    size_t bpp = 1;
    if (fmt_ == UHDR_IMG_FMT_24bppRGB888) bpp = 3;
    else if (fmt_ == UHDR_IMG_FMT_32bppRGBA8888 || fmt_ == UHDR_IMG_FMT_32bppRGBA1010102) bpp = 4;
    else if (fmt_ == UHDR_IMG_FMT_64bppRGBAHalfFloat) bpp = 8;
    block_.reset(static_cast<uint8_t*>(std::calloc((size_t)aligned_w * h_ * bpp + 64, 1)));
    planes[0] = block_.get();
    stride[0] = aligned_w;
  }

 private:
  struct free_deleter {
    void operator()(uint8_t* p) const { std::free(p); }
  };
  std::unique_ptr<uint8_t, free_deleter> block_;
};

class UltraHdr {
 public:
  // ultrahdrcommon.h:450-457 (Android defaults: scale 4, quality 85, single channel, REALTIME)
  explicit UltraHdr(int device = -1, int mapDimensionScaleFactor = 4, int mapCompressQuality = 85,
                    bool useMultiChannelGainMap = false, float gamma = 1.0f,
                    uhdr_enc_preset_t preset = UHDR_USAGE_REALTIME, float minContentBoost = FLT_MIN,
                    float maxContentBoost = FLT_MAX, float targetDispPeakBrightness = -1.0f)
      : mMapDimensionScaleFactor(mapDimensionScaleFactor),
        mMapCompressQuality(mapCompressQuality),
        mUseMultiChannelGainMap(useMultiChannelGainMap),
        mGamma(gamma),
        mEncPreset(preset),
        mMinContentBoost(minContentBoost),
        mMaxContentBoost(maxContentBoost),
        mTargetDispPeakBrightness(targetDispPeakBrightness) {
    mCtx = uhdr_hip_create(device, &mCreateStatus);
  }
  ~UltraHdr() {
    if (mCtx) uhdr_hip_destroy(mCtx);
  }
  UltraHdr(const UltraHdr&) = delete;
  UltraHdr& operator=(const UltraHdr&) = delete;

  // UHDR_CODEC_OK, or why no MI355X-class device could be opened (there is no CPU fallback)
  uhdr_error_info_t status() const { return mCreateStatus; }
  uhdr_hip_ctx_t* context() const { return mCtx; }

  uhdr_error_info_t toneMap(uhdr_raw_image_t* hdr_intent, uhdr_raw_image_t* sdr_intent) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_tone_map(mCtx, hdr_intent, sdr_intent);
  }

  uhdr_error_info_t generateGainMap(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent,
                                    uhdr_gainmap_metadata_t* gainmap_metadata, std::unique_ptr<raw_image_ext>& gainmap_img,
                                    bool sdr_is_601 = false, bool use_luminance = true) {
    return generateGainMapEx(sdr_intent, hdr_intent, gainmap_metadata, gainmap_img, 0u, sdr_is_601, use_luminance);
  }

  // generateGainMap with flags: 0 is uhdr_hip_generate_gainmap, anything else goes to uhdr_hip_generate_gainmap_ex --
  // UHDR_HIP_GENERATE_GAMMA_TABLE runs a gain-map gamma other than 1 through the host-built byte thresholds instead of a pow per sample
  // (gainmapmath.cpp:769-770, 784-789): the reference's bytes.
  uhdr_error_info_t generateGainMapEx(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_gainmap_metadata_t* gainmap_metadata,
                                      std::unique_ptr<raw_image_ext>& gainmap_img, unsigned int flags, bool sdr_is_601 = false,
                                      bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    if (!sdr_intent || !hdr_intent || !gainmap_metadata) return bad("received nullptr argument");
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0,
                              use_luminance ? 1 : 0};
    // map geometry: jpegr.cpp:693-716
    unsigned scale = mMapDimensionScaleFactor < 1 ? 1u : (unsigned)mMapDimensionScaleFactor;
    unsigned mw = sdr_intent->w / scale, mh = sdr_intent->h / scale;
    if (mw == 0 || mh == 0) {
      unsigned s = sdr_intent->w < sdr_intent->h ? sdr_intent->w : sdr_intent->h;
      s = s >= 8 ? s / 8 : 1;
      mw = sdr_intent->w / s;
      mh = sdr_intent->h / s;
    }
    gainmap_img = std::make_unique<raw_image_ext>(mUseMultiChannelGainMap ? UHDR_IMG_FMT_24bppRGB888 : UHDR_IMG_FMT_8bppYCbCr400,
                                                  hdr_intent->cg, hdr_intent->ct, hdr_intent->range, mw, mh, 64);
    if (flags == 0u) return uhdr_hip_generate_gainmap(mCtx, sdr_intent, hdr_intent, &cfg, gainmap_metadata, gainmap_img.get());
    return uhdr_hip_generate_gainmap_ex(mCtx, sdr_intent, hdr_intent, &cfg, gainmap_metadata, gainmap_img.get(), flags);
  }

  uhdr_error_info_t applyGainMap(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* gainmap_img,
                                 uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                 uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_apply_gainmap(mCtx, sdr_intent, gainmap_img, gainmap_metadata, output_ct, output_format, max_display_boost, dest);
  }

  // applyGainMap including the reference's resize step for a gain map of another aspect ratio (jpegr.cpp:1651-1671,
  // uhdr_hip_apply_gainmap_any); applyGainMap above keeps refusing such a map.
  uhdr_error_info_t applyGainMapAny(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* gainmap_img,
                                    uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                    uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_apply_gainmap_any(mCtx, sdr_intent, gainmap_img, gainmap_metadata, output_ct, output_format, max_display_boost, dest);
  }

  // applyGainMap with flags (uhdr_hip_apply_gainmap_ex): UHDR_HIP_APPLY_RESIZED_MAP is applyGainMapAny, UHDR_HIP_APPLY_GAMMA_TABLE
  // evaluates a gain-map gamma other than 1 (GainLUT::getGainFactor, gainmapmath.h:483-489) through host-built thresholds
  // instead of a pow per sample -- the reference's bits; 0 is applyGainMap.
  uhdr_error_info_t applyGainMapEx(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* gainmap_img,
                                   uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                   uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest, unsigned int flags) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_apply_gainmap_ex(mCtx, sdr_intent, gainmap_img, gainmap_metadata, output_ct, output_format, max_display_boost, dest, flags);
  }

  // resize_image (editorhelper.cpp:88-146) for Y400 / RGB888 / RGBA8888 into a caller-provided image of the wanted size
  uhdr_error_info_t resizeImage(uhdr_raw_image_t* src, uhdr_raw_image_t* dst) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_resize_image(mCtx, src, dst);
  }

  // applyGainMap on a base image still in coefficient form (device pointers; gainmap_img and dest are device images): the
  // dequantize + IDCT stage runs inside the kernel.  sampling422: the coefficients are a 4:2:2 frame's, not a 4:2:0 one's.
  uhdr_error_info_t applyGainMapFromCoefficients(const uhdr_hip_jpeg_coefficients_t* base, unsigned int w, unsigned int h,
                                                 uhdr_color_gamut_t base_cg, uhdr_raw_image_t* gainmap_img,
                                                 uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                                 uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest,
                                                 bool sampling422 = false) {
    if (!mCtx) return mCreateStatus;
    return sampling422 ? uhdr_hip_apply_gainmap_coef422_dev(mCtx, base, w, h, base_cg, gainmap_img, gainmap_metadata, output_ct, output_format,
                                                            max_display_boost, dest)
                       : uhdr_hip_apply_gainmap_coef_dev(mCtx, base, w, h, base_cg, gainmap_img, gainmap_metadata, output_ct, output_format,
                                                         max_display_boost, dest);
  }

  // ... of a 4:4:4 frame (uhdr_hip_apply_gainmap_coef444_dev): all three components on the ceil(w/8) x ceil(h/8) block grid.
  uhdr_error_info_t applyGainMapFromCoefficients444(const uhdr_hip_jpeg_coefficients_t* base, unsigned int w, unsigned int h,
                                                    uhdr_color_gamut_t base_cg, uhdr_raw_image_t* gainmap_img,
                                                    uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                                    uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_apply_gainmap_coef444_dev(mCtx, base, w, h, base_cg, gainmap_img, gainmap_metadata, output_ct, output_format,
                                              max_display_boost, dest);
  }

  // ... of any sampling (420, 422 or 444) with applyGainMapEx's flags (uhdr_hip_apply_gainmap_coef_ex_dev; gainmapmath.h:483-489):
  // with UHDR_HIP_APPLY_GAMMA_TABLE a gamma other than 1 at an even map scale <= 8 stays on the coefficient kernel.
  uhdr_error_info_t applyGainMapFromCoefficientsEx(const uhdr_hip_jpeg_coefficients_t* base, int sampling, unsigned int w, unsigned int h,
                                                   uhdr_color_gamut_t base_cg, uhdr_raw_image_t* gainmap_img,
                                                   uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_color_transfer_t output_ct,
                                                   uhdr_img_fmt_t output_format, float max_display_boost, uhdr_raw_image_t* dest,
                                                   unsigned int flags) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_apply_gainmap_coef_ex_dev(mCtx, base, sampling, w, h, base_cg, gainmap_img, gainmap_metadata, output_ct, output_format,
                                              max_display_boost, dest, flags);
  }

  // decodeApi1ScansAny below with applyGainMapEx's flags for its applyGainMap stage (uhdr_hip_decode_api1_scans_ex_dev; gainmapmath.h:483-489)
  uhdr_error_info_t decodeApi1ScansEx(const uhdr_hip_jpeg_header_t* base, const uint8_t* base_data, size_t base_bytes,
                                      uhdr_color_gamut_t base_cg, const uhdr_hip_jpeg_header_t* map, const uint8_t* map_data,
                                      size_t map_bytes, uhdr_color_gamut_t map_cg, uhdr_gainmap_metadata_t* gainmap_metadata,
                                      uhdr_color_transfer_t output_ct, uhdr_img_fmt_t output_format, float max_display_boost,
                                      uhdr_raw_image_t* dest, unsigned int apply_flags, int libjpeg_variant = 0) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_decode_api1_scans_ex_dev(mCtx, base, base_data, base_bytes, base_cg, map, map_data, map_bytes, map_cg, libjpeg_variant,
                                             gainmap_metadata, output_ct, output_format, max_display_boost, dest, apply_flags);
  }

  // JpegR::decodeJPEGR behind its container parsing on device data in one call (uhdr_hip_decode_api1_scans_any_dev): two parsed
  // headers + their entropy-coded bytes in device memory -> dest (device image).  The base scan is 4:2:0, 4:2:2 or 4:4:4.
  uhdr_error_info_t decodeApi1ScansAny(const uhdr_hip_jpeg_header_t* base, const uint8_t* base_data, size_t base_bytes,
                                       uhdr_color_gamut_t base_cg, const uhdr_hip_jpeg_header_t* map, const uint8_t* map_data,
                                       size_t map_bytes, uhdr_color_gamut_t map_cg, uhdr_gainmap_metadata_t* gainmap_metadata,
                                       uhdr_color_transfer_t output_ct, uhdr_img_fmt_t output_format, float max_display_boost,
                                       uhdr_raw_image_t* dest, int libjpeg_variant = 0) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_decode_api1_scans_any_dev(mCtx, base, base_data, base_bytes, base_cg, map, map_data, map_bytes, map_cg, libjpeg_variant,
                                              gainmap_metadata, output_ct, output_format, max_display_boost, dest);
  }

  // toneMap (P010 -> YCbCr 4:2:0) + generateGainMap of an API-0 encode in one pass over a device-resident P010 intent
  // (uhdr_hip_encode_api0_p010_fused_dev): base_ycc420 and gainmap_img are device images the caller allocated; scale factor 1.
  uhdr_error_info_t encodeApi0FusedP010(uhdr_raw_image_t* hdr_intent, uhdr_raw_image_t* base_ycc420, uhdr_gainmap_metadata_t* gainmap_metadata,
                                        uhdr_raw_image_t* gainmap_img, bool use_luminance = false) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api0_p010_fused_dev(mCtx, hdr_intent, &cfg, base_ycc420, gainmap_metadata, gainmap_img);
  }

  // JpegR::encodeJPEGR API-0 without the container in one call (uhdr_hip_encode_api0_scans_any): a host RGBA1010102, RGBA half-float or
  // P010 intent -> the two entropy-coded scans in host buffers.  qt_base / qt_map: {luma, chroma} tables.
  uhdr_error_info_t encodeApi0ScansAny(uhdr_raw_image_t* hdr_intent, const uint16_t qt_base[2][64], const uint16_t qt_map[2][64],
                                       uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_desc, uhdr_color_gamut_t* sdr_cg,
                                       uint8_t* base_scan, size_t base_capacity, size_t* base_bytes, uint8_t* map_scan, size_t map_capacity,
                                       size_t* map_bytes) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, 0};
    return uhdr_hip_encode_api0_scans_any(mCtx, hdr_intent, &cfg, qt_base, qt_map, gainmap_metadata, gainmap_desc, sdr_cg, base_scan, base_capacity,
                                          base_bytes, map_scan, map_capacity, map_bytes);
  }

  // The API-0 front ends for a gain map at scale factor 1, 2 or 4 (uhdr_hip_encode_api0_fused_scaled_dev for RGBA1010102 / RGBA half-float
  // intents, uhdr_hip_encode_api0_p010_fused_scaled_dev for P010): device images the caller allocated, gainmap_img of (w / S) x (h / S) pixels;
  // sdr_rgba may be null.  Scale factor 2 / 4: one pass (UHDR_USAGE_REALTIME), RGBA1010102 or P010.
  uhdr_error_info_t encodeApi0FusedScaled(uhdr_raw_image_t* hdr_intent, uhdr_raw_image_t* sdr_rgba, uhdr_raw_image_t* base_ycc,
                                          uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_img, bool use_luminance = false) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api0_fused_scaled_dev(mCtx, hdr_intent, &cfg, sdr_rgba, base_ycc, gainmap_metadata, gainmap_img);
  }
  uhdr_error_info_t encodeApi0FusedP010Scaled(uhdr_raw_image_t* hdr_intent, uhdr_raw_image_t* base_ycc420, uhdr_gainmap_metadata_t* gainmap_metadata,
                                              uhdr_raw_image_t* gainmap_img, bool use_luminance = false) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api0_p010_fused_scaled_dev(mCtx, hdr_intent, &cfg, base_ycc420, gainmap_metadata, gainmap_img);
  }

  // encodeApi0ScansAny for a gain map at scale factor 1, 2 or 4 (uhdr_hip_encode_api0_scans_scaled): 2 and 4 for RGBA1010102 and P010 intents
  // whose map is whole 8 x 8 blocks; gainmap_desc carries the map's dimensions.
  uhdr_error_info_t encodeApi0ScansScaled(uhdr_raw_image_t* hdr_intent, const uint16_t qt_base[2][64], const uint16_t qt_map[2][64],
                                          uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_desc, uhdr_color_gamut_t* sdr_cg,
                                          uint8_t* base_scan, size_t base_capacity, size_t* base_bytes, uint8_t* map_scan, size_t map_capacity,
                                          size_t* map_bytes) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, 0};
    return uhdr_hip_encode_api0_scans_scaled(mCtx, hdr_intent, &cfg, qt_base, qt_map, gainmap_metadata, gainmap_desc, sdr_cg, base_scan, base_capacity,
                                             base_bytes, map_scan, map_capacity, map_bytes);
  }

  // encodeApi0ScansScaled for frames that are not whole MCUs and maps that are not whole blocks as well -- 1920 x 1080 P010
  // (uhdr_hip_encode_api0_scans_edges); the scans carry the real blocks of the true w x h.
  // encodeApi0ScansEdgesDev (uhdr_hip_encode_api0_scans_edges_dev): the intent's planes and both scan buffers are device memory.
  uhdr_error_info_t encodeApi0ScansEdges(uhdr_raw_image_t* hdr_intent, const uint16_t qt_base[2][64], const uint16_t qt_map[2][64],
                                         uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_desc, uhdr_color_gamut_t* sdr_cg,
                                         uint8_t* base_scan, size_t base_capacity, size_t* base_bytes, uint8_t* map_scan, size_t map_capacity,
                                         size_t* map_bytes, bool dev = false) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 0, 0};
    return (dev ? uhdr_hip_encode_api0_scans_edges_dev : uhdr_hip_encode_api0_scans_edges)(mCtx, hdr_intent, &cfg, qt_base, qt_map, gainmap_metadata, gainmap_desc,
                                                                                          sdr_cg, base_scan, base_capacity, base_bytes, map_scan, map_capacity,
                                                                                          map_bytes);
  }
  uhdr_error_info_t encodeApi0ScansEdgesDev(uhdr_raw_image_t* hdr_intent, const uint16_t qt_base[2][64], const uint16_t qt_map[2][64],
                                            uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_desc, uhdr_color_gamut_t* sdr_cg,
                                            uint8_t* base_scan, size_t base_capacity, size_t* base_bytes, uint8_t* map_scan, size_t map_capacity,
                                            size_t* map_bytes) {
    return encodeApi0ScansEdges(hdr_intent, qt_base, qt_map, gainmap_metadata, gainmap_desc, sdr_cg, base_scan, base_capacity, base_bytes, map_scan,
                                map_capacity, map_bytes, /*dev=*/true);
  }

  // The sample -> coefficient part of an API-1 encode on device-resident intents (uhdr_hip_encode_api1_fused_any_dev): the SDR intent is
  // YCbCr 4:2:0 (multiples of 16) or RGBA8888 (multiples of 8; its base image is 4:4:4, three (w/8)*(h/8) coefficient arrays).
  // blocks: device buffers; gainmap_img may be null.
  uhdr_error_info_t encodeApi1FusedAny(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                       const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], const uhdr_hip_api1_blocks_t* blocks,
                                       uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_img, bool sdr_is_601 = false,
                                       bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api1_fused_any_dev(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base, qt_map, blocks, gainmap_metadata, gainmap_img);
  }

  // JpegR::encodeJPEGR API-1 without the container in one call, for a YCbCr 4:2:0 or an RGBA8888 SDR intent (base scan 1x1 / 1x1 / 1x1):
  // dev == false: host intents and host scan buffers (uhdr_hip_encode_api1_scans_any); dev == true: device intents and device buffers
  // (uhdr_hip_encode_api1_scans_any_dev).  qt_base / qt_map: {luma, chroma} tables.
  uhdr_error_info_t encodeApi1ScansAny(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                       const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], uhdr_gainmap_metadata_t* gainmap_metadata,
                                       uhdr_raw_image_t* gainmap_desc, uint8_t* base_scan, size_t base_capacity, size_t* base_bytes,
                                       uint8_t* map_scan, size_t map_capacity, size_t* map_bytes, bool dev = false, bool sdr_is_601 = false,
                                       bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return (dev ? uhdr_hip_encode_api1_scans_any_dev : uhdr_hip_encode_api1_scans_any)(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base, qt_map,
                                                                                       gainmap_metadata, gainmap_desc, base_scan, base_capacity,
                                                                                       base_bytes, map_scan, map_capacity, map_bytes);
  }

  // encodeApi1FusedAny / encodeApi1ScansAny for the one-pass preset as well (uhdr_hip_encode_api1_fused_onepass_dev,
  // uhdr_hip_encode_api1_scans_onepass / _onepass_dev): UHDR_USAGE_REALTIME is two launches -- both intents to the map's coefficients, the base
  // image's blocks -- at any scale factor whose map is whole 8 x 8 blocks; UHDR_USAGE_BEST_QUALITY runs what the siblings run.
  uhdr_error_info_t encodeApi1FusedOnePass(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                           const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], const uhdr_hip_api1_blocks_t* blocks,
                                           uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_img, bool sdr_is_601 = false,
                                           bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api1_fused_onepass_dev(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base, qt_map, blocks, gainmap_metadata, gainmap_img);
  }
  uhdr_error_info_t encodeApi1ScansOnePass(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                           const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], uhdr_gainmap_metadata_t* gainmap_metadata,
                                           uhdr_raw_image_t* gainmap_desc, uint8_t* base_scan, size_t base_capacity, size_t* base_bytes,
                                           uint8_t* map_scan, size_t map_capacity, size_t* map_bytes, bool dev = false, bool sdr_is_601 = false,
                                           bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return (dev ? uhdr_hip_encode_api1_scans_onepass_dev : uhdr_hip_encode_api1_scans_onepass)(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base,
                                                                                               qt_map, gainmap_metadata, gainmap_desc, base_scan,
                                                                                               base_capacity, base_bytes, map_scan, map_capacity, map_bytes);
  }
  // encodeApi1ScansOnePass with generateGainMap's flags (uhdr_hip_encode_api1_scans_ex / _ex_dev): with UHDR_HIP_GENERATE_GAMMA_TABLE a gain-map
  // gamma other than 1 keeps the fused chain, both presets; flags 0 is encodeApi1ScansOnePass.
  uhdr_error_info_t encodeApi1ScansEx(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                      const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], uhdr_gainmap_metadata_t* gainmap_metadata,
                                      uhdr_raw_image_t* gainmap_desc, uint8_t* base_scan, size_t base_capacity, size_t* base_bytes,
                                      uint8_t* map_scan, size_t map_capacity, size_t* map_bytes, unsigned int flags, bool dev = false,
                                      bool sdr_is_601 = false, bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return (dev ? uhdr_hip_encode_api1_scans_ex_dev : uhdr_hip_encode_api1_scans_ex)(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base, qt_map,
                                                                                     gainmap_metadata, gainmap_desc, base_scan, base_capacity, base_bytes,
                                                                                     map_scan, map_capacity, map_bytes, flags);
  }
  // encodeApi1FusedOnePass / encodeApi1ScansEx for frames that are not whole MCUs and maps that are not whole blocks -- 1920 x 1080, 4000 x 3000
  // (uhdr_hip_encode_api1_fused_edges_dev, uhdr_hip_encode_api1_scans_edges / _edges_dev; jpegencoderhelper.cpp:246-309): a 4:2:0 SDR intent of
  // any even size, a map of any size, coefficient arrays on libjpeg's width_in_blocks grids.  What the siblings take runs what they run.
  uhdr_error_info_t encodeApi1FusedEdges(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                         const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], const uhdr_hip_api1_blocks_t* blocks,
                                         uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_img, unsigned int flags = 0,
                                         bool sdr_is_601 = false, bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return uhdr_hip_encode_api1_fused_edges_dev(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base, qt_map, blocks, gainmap_metadata, gainmap_img,
                                                flags);
  }
  uhdr_error_info_t encodeApi1ScansEdges(uhdr_raw_image_t* sdr_intent, uhdr_raw_image_t* hdr_intent, uhdr_color_gamut_t base_encoding,
                                         const uint16_t qt_base[2][64], const uint16_t qt_map[2][64], uhdr_gainmap_metadata_t* gainmap_metadata,
                                         uhdr_raw_image_t* gainmap_desc, uint8_t* base_scan, size_t base_capacity, size_t* base_bytes,
                                         uint8_t* map_scan, size_t map_capacity, size_t* map_bytes, unsigned int flags = 0, bool dev = false,
                                         bool sdr_is_601 = false, bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return (dev ? uhdr_hip_encode_api1_scans_edges_dev : uhdr_hip_encode_api1_scans_edges)(mCtx, sdr_intent, hdr_intent, &cfg, base_encoding, qt_base,
                                                                                           qt_map, gainmap_metadata, gainmap_desc, base_scan, base_capacity,
                                                                                           base_bytes, map_scan, map_capacity, map_bytes, flags);
  }

  // generateGainMap on an SDR intent still in coefficient form -- the compressed intent of an API-3 encode after its Huffman decode (device
  // pointers; hdr_intent and gainmap_img are device images): the dequantize + IDCT stage runs inside the kernel
  // (uhdr_hip_generate_gainmap_coef_dev; sampling422: uhdr_hip_generate_gainmap_coef422_dev).  == idct_dequant x 3 + generateGainMap.
  uhdr_error_info_t generateGainMapFromCoefficients(const uhdr_hip_jpeg_coefficients_t* sdr, unsigned int w, unsigned int h, uhdr_color_gamut_t sdr_cg,
                                                    uhdr_raw_image_t* hdr_intent, uhdr_gainmap_metadata_t* gainmap_metadata, uhdr_raw_image_t* gainmap_img,
                                                    bool sampling422 = false, bool sdr_is_601 = false, bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return (sampling422 ? uhdr_hip_generate_gainmap_coef422_dev : uhdr_hip_generate_gainmap_coef_dev)(mCtx, sdr, w, h, sdr_cg, hdr_intent, &cfg,
                                                                                                      gainmap_metadata, gainmap_img);
  }

  // ... of a 4:4:4 frame (uhdr_hip_generate_gainmap_coef444_dev): all three components on the ceil(w/8) x ceil(h/8) block grid.
  uhdr_error_info_t generateGainMapFromCoefficients444(const uhdr_hip_jpeg_coefficients_t* sdr, unsigned int w, unsigned int h, uhdr_color_gamut_t sdr_cg,
                                                       uhdr_raw_image_t* hdr_intent, uhdr_gainmap_metadata_t* gainmap_metadata,
                                                       uhdr_raw_image_t* gainmap_img, bool sdr_is_601 = false, bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, sdr_is_601 ? 1 : 0, use_luminance ? 1 : 0};
    return uhdr_hip_generate_gainmap_coef444_dev(mCtx, sdr, w, h, sdr_cg, hdr_intent, &cfg, gainmap_metadata, gainmap_img);
  }

  // JpegR::encodeJPEGR API-3 (jpegr.cpp:327-385) without the container in one call (uhdr_hip_encode_api3_scans / _dev): the compressed SDR
  // intent's parsed header and entropy-coded bytes + the raw HDR intent -> the gain map's scan.  The base image stays the caller's JPEG.
  uhdr_error_info_t encodeApi3Scans(const uhdr_hip_jpeg_header_t* sdr_jpeg, const uint8_t* sdr_data, size_t sdr_bytes, uhdr_color_gamut_t sdr_cg,
                                    uhdr_raw_image_t* hdr_intent, const uint16_t qt_map[2][64], uhdr_gainmap_metadata_t* gainmap_metadata,
                                    uhdr_raw_image_t* gainmap_desc, uint8_t* map_scan, size_t map_capacity, size_t* map_bytes, bool dev = false,
                                    bool use_luminance = true) {
    if (!mCtx) return mCreateStatus;
    uhdr_hip_encode_cfg_t cfg{mMapDimensionScaleFactor, mUseMultiChannelGainMap ? 1 : 0, mGamma, (int)mEncPreset,
                              mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness, 1, use_luminance ? 1 : 0};
    return (dev ? uhdr_hip_encode_api3_scans_dev : uhdr_hip_encode_api3_scans)(mCtx, sdr_jpeg, sdr_data, sdr_bytes, sdr_cg, hdr_intent, &cfg, qt_map,
                                                                               gainmap_metadata, gainmap_desc, map_scan, map_capacity, map_bytes);
  }

  uhdr_error_info_t convertYuv(uhdr_raw_image_t* image, uhdr_color_gamut_t src_encoding, uhdr_color_gamut_t dst_encoding) {
    if (!mCtx) return mCreateStatus;
    return uhdr_hip_convert_yuv(mCtx, image, src_encoding, dst_encoding);
  }

 protected:
  void setMapDimensionScaleFactor(int v) { mMapDimensionScaleFactor = v; }
  int getMapDimensionScaleFactor() const { return mMapDimensionScaleFactor; }
  void setMapCompressQuality(int v) { mMapCompressQuality = v; }
  int getMapCompressQuality() const { return mMapCompressQuality; }
  void setGainMapGamma(float v) { mGamma = v; }
  float getGainMapGamma() const { return mGamma; }
  void setUseMultiChannelGainMap(bool v) { mUseMultiChannelGainMap = v; }
  bool isUsingMultiChannelGainMap() const { return mUseMultiChannelGainMap; }
  void setGainMapMinMaxContentBoost(float mn, float mx) { mMinContentBoost = mn; mMaxContentBoost = mx; }

 private:
  static uhdr_error_info_t bad(const char* msg) {
    uhdr_error_info_t st;
    std::memset(&st, 0, sizeof st);
    st.error_code = UHDR_CODEC_INVALID_PARAM;
    st.has_detail = 1;
    std::strncpy(st.detail, msg, sizeof st.detail - 1);
    return st;
  }
  uhdr_hip_ctx_t* mCtx = nullptr;
  uhdr_error_info_t mCreateStatus{};
  int mMapDimensionScaleFactor;
  int mMapCompressQuality;
  bool mUseMultiChannelGainMap;
  float mGamma;
  uhdr_enc_preset_t mEncPreset;
  float mMinContentBoost, mMaxContentBoost, mTargetDispPeakBrightness;
};

}  // namespace uhdr_hip
