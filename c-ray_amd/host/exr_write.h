/* exr_write.h — the host side of the multi-layer OpenEXR output, in C for the drop-in program: a single-part scanline file whose channels are
 * FLOAT or HALF — uncompressed, or ZIP / ZIPS from chunks deflated on the device —, and Cryptomatte's naming of ids. The pixel data comes packed from the libraries
 * (crh_pack_scanlines, include/cray_hip.h; crx_pack, include/cray_hip_exr.h); this file knows which channel of
 * which buffer carries which name and writes what goes around the data. c-ray_amd/exr.py states the same in Python; both write the same bytes. Not part of the
 * library. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "cray_hip.h"

#define EXR_MAX_NAME 31          /* attribute and channel names of a file without the long-names bit */
#define EXR_CRYPTO_RANKS 6       /* crh_ids_resolve's ranks: three RGBA layers of two (id, coverage) pairs */

uint32_t exr_murmur3_32(const void *data, size_t len, uint32_t seed);
/* the word a Cryptomatte id channel holds for a name: its hash, bit 23 flipped where the exponent field is 0 or 255 (uint32_to_float32) */
uint32_t exr_crypto_id(const char *name);

/* a string attribute; exr_crypto_attrs allocates both members, exr_free_attrs frees them */
struct exr_attr { char *name, *value; };
/* the four cryptomatte/<key>/... attributes of a layer whose id i is called names[i] (unique names); 0, or -1 when out of memory */
int exr_crypto_attrs(const char *layer, const char *const *names, uint32_t count, struct exr_attr out[4]);
void exr_free_attrs(struct exr_attr *attrs, int count);

/* The channels of the layers whose buffer is given (fb is always there), in ascending byte order of name — the order of the file's channel list and of the pack:
 * R G B from fb; albedo.R/G/B normal.X/Y/Z Z A from an AOV buffer; denoised.R/G/B; CryptoObject00..02.R/G/B/A and CryptoMaterial00..02.R/G/B/A from
 * crh_ids_resolve's outputs, the id channels mapped through instance_map / material_map. names[i] points at storage of this file. Returns the count (<= 38). */
int exr_layer_channels(const float *fb, const float *aov, const float *denoised, const float *instance_ranked, const float *material_ranked,
                       const uint32_t *instance_map, uint32_t instance_count, const uint32_t *material_map, uint32_t material_count,
                       crh_pack_channel channels[CRH_PACK_MAX_CHANNELS], const char *names[CRH_PACK_MAX_CHANNELS]);

/* Pixel types as crx_pack takes them (CRX_PIXEL_FLOAT / CRX_PIXEL_HALF of include/cray_hip_exr.h); the file's channel list says 2 and 1. */
#define EXR_FLOAT 0
#define EXR_HALF 1

/* The file: header (channel names in ascending byte order, a pixel type per channel — pixel_types NULL: all FLOAT —; the fixed attributes and `strings`, sorted
 * here), offset table, and `chunk_data` — the chunks back to back as crx_pack writes them (include/cray_hip_exr.h), chunk k of chunk_sizes[k] bytes — verbatim.
 * compression 0 (a raw chunk a row: where all channels are FLOAT, crh_pack_scanlines' blocks of 8 + 4 * channel_count * width bytes), 2 (ZIPS: a chunk a row) or
 * 3 (ZIP: a chunk every 16 rows); the offset table has chunk_count = ceil(height / 1 or 16) entries. 0, or -1 (a name too long or out of order, a pixel type that
 * is neither, another compression, a chunk count that does not fit the height, a chunk of less than 8 bytes, out of memory, the file). Same bytes as exr.file_bytes. */
int exr_write_file(const char *path, int width, int height, const char *const *channel_names, const uint8_t *pixel_types, int channel_count,
                   const struct exr_attr *strings, int string_count, int compression, const void *chunk_data, const uint64_t *chunk_sizes, int chunk_count);

/* CRAY_HIP_EXR_HALF=1's default set, as Context.write_layers_exr(half=True) chooses it: pixel_types[c] = EXR_HALF for R G B, albedo.R/G/B, normal.X/Y/Z and
 * denoised.R/G/B, EXR_FLOAT for everything else (Z, A, the Cryptomatte channels). Returns how many are HALF. */
int exr_half_types(const char *const *channel_names, int channel_count, uint8_t *pixel_types);
