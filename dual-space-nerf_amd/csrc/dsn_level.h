// dsn_level.h - the image writers' float -> level rule (dsn_jpeg.hip, dsn_pnge.hip; "Levels" in include/dsnerf.h): ONE definition, so
// that a .jpg and a .png of the same frame start from the same 8-bit levels.
#pragma once
#include "../../include/dsnerf.h"

// element idx of an image of dtype DSN_JPEG_U8 / DSN_JPEG_F32: uint8 passes through; float32 v: v * scale in float32, nearest-even,
// saturated to [0, 255], NaN -> 0; `bad` is raised by a NaN or an infinite v
__device__ __forceinline__ int dsn_image_level(const void* __restrict__ img, int dtype, size_t idx, float scale, bool& bad) {
    if (dtype == DSN_JPEG_U8) return ((const uint8_t*)img)[idx];
    const float v = ((const float*)img)[idx];
    if (!(fabsf(v) <= 3.402823466e38f)) bad = true;              // NaN or infinite
    const float t = v * scale;
    if (!(t == t)) return 0;                                      // NaN (of v, or of 0 x inf) gives 0
    const float r = rintf(t);                                     // half to even
    return r <= 0.0f ? 0 : r >= 255.0f ? 255 : (int)r;
}
