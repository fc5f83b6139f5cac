/*
 * srgb8.h — THE statement of how a frame's float becomes the byte of the 8-bit picture: the reference's colorToSRGB (color.h:51-84) and setPixel's truncation
 * (texture.c:18-22). Included by pt_device.h (libcray_hip.so: k_to_srgb8, crh_framebuffer_to_srgb8) and by png_pack.h (libcray_hip_exr.so: crx_png_pack), so
 * that the PNG the companion library writes holds, byte for byte, what crh_framebuffer_to_srgb8 gives. Device and host like exact_math.h, which it needs for powf's
 * bits. The contract covers finite values >= 0, values above 1 included: what a frame holds.
 */
#pragma once
#include "exact_math.h"

namespace crh {

CRH_EM float linearToSRGB(float c) {                                                                /* color.h:51 */
	if (c <= 0.0031308f) return 12.92f * c;
	return (1.055f * em::powf_(c, 0.4166666667f)) - 0.055f;
}
/* texture.c:18-22: (unsigned char)min(v * 255, 255) of the sRGB value */
CRH_EM unsigned char linearToSRGB8(float c) {
	const float v = linearToSRGB(c) * 255.0f;
	return (unsigned char)(v < 255.0f ? v : 255.0f);
}

}  // namespace crh
