/* exr_write.c — see exr_write.h. The layout, for a reader of this file alone:
 *   magic 76 2f 31 01, version 02 00 00 00 (single part, scanline, short names);
 *   attributes in ascending byte order of name, each `name\0 type\0 int32 size, value`: channels (chlist: per channel name\0, int32 pixelType 2 = FLOAT or 1 = HALF, uint8 pLinear 0,
 *   three zero bytes, int32 xSampling 1, int32 ySampling 1; one \0 ends the list), compression (one byte: 0, 2 ZIPS or 3 ZIP), dataWindow and displayWindow (box2i 0, 0, W - 1, H - 1),
 *   lineOrder (one byte 0: increasing y, stored row 0 is y 0), pixelAspectRatio (float 1), screenWindowCenter (v2f 0, 0), screenWindowWidth (float 1), the string
 *   attributes (size = length, no terminator); one \0 ends the header;
 *   one uint64 absolute offset per chunk of 1 (compression 0, ZIPS) or 16 (ZIP) rows; the chunks as crx_pack writes them (include/cray_hip_exr.h: int32 y, int32 size,
 *   the data). Compression 0: a raw chunk a row, which where all channels are FLOAT is crh_pack_scanlines' block.
 * Little-endian throughout, written byte by byte. */
#include "exr_write.h"

#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

uint32_t exr_murmur3_32(const void *data, size_t len, uint32_t seed) {
	const unsigned char *p = data;
	const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
	uint32_t h = seed;
	size_t i = 0;
	for (; i + 4 <= len; i += 4) {
		uint32_t k = (uint32_t)p[i] | (uint32_t)p[i + 1] << 8 | (uint32_t)p[i + 2] << 16 | (uint32_t)p[i + 3] << 24;
		k *= c1; k = rotl32(k, 15); k *= c2;
		h ^= k; h = rotl32(h, 13); h = h * 5u + 0xe6546b64u;
	}
	uint32_t k = 0;
	for (size_t j = len; j > i; --j) k = k << 8 | p[j - 1];
	if (len > i) { k *= c1; k = rotl32(k, 15); k *= c2; h ^= k; }
	h ^= (uint32_t)len;
	h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
	return h;
}

uint32_t exr_crypto_id(const char *name) {
	uint32_t h = exr_murmur3_32(name, strlen(name), 0);
	const uint32_t e = (h >> 23) & 255u;
	if (e == 0u || e == 255u) h ^= 1u << 23;
	return h;
}

/* a growing byte string; `failed` sticks */
struct bytes { unsigned char *p; size_t n, cap; int failed; };
static void put(struct bytes *b, const void *src, size_t n) {
	if (b->failed) return;
	if (b->n + n > b->cap) {
		size_t cap = b->cap ? b->cap : 256;
		while (cap < b->n + n) cap *= 2;
		unsigned char *q = realloc(b->p, cap);
		if (!q) { b->failed = 1; return; }
		b->p = q; b->cap = cap;
	}
	memcpy(b->p + b->n, src, n);
	b->n += n;
}
static void put_str(struct bytes *b, const char *s) { put(b, s, strlen(s)); }
static void put_u32(struct bytes *b, uint32_t v) {
	const unsigned char w[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
	put(b, w, 4);
}
static void put_u64(struct bytes *b, uint64_t v) { put_u32(b, (uint32_t)v); put_u32(b, (uint32_t)(v >> 32)); }
static void put_attr(struct bytes *b, const char *name, const char *type, const void *value, size_t size) {
	put(b, name, strlen(name) + 1);
	put(b, type, strlen(type) + 1);
	put_u32(b, (uint32_t)size);
	put(b, value, size);
}

/* a JSON string the way Python's json.dumps(ensure_ascii=False) writes it: \" \\ \b \f \n \r \t, \u00xx for the other control characters, UTF-8 as it is */
static void put_json_string(struct bytes *b, const char *s) {
	put(b, "\"", 1);
	for (; *s; ++s) {
		const unsigned char c = (unsigned char)*s;
		char esc[8];
		if (c == '"') put_str(b, "\\\"");
		else if (c == '\\') put_str(b, "\\\\");
		else if (c == '\b') put_str(b, "\\b");
		else if (c == '\f') put_str(b, "\\f");
		else if (c == '\n') put_str(b, "\\n");
		else if (c == '\r') put_str(b, "\\r");
		else if (c == '\t') put_str(b, "\\t");
		else if (c < 0x20) { snprintf(esc, sizeof(esc), "\\u%04x", c); put_str(b, esc); }
		else put(b, &c, 1);
	}
	put(b, "\"", 1);
}

static char *dup_str(const char *s) {
	char *d = malloc(strlen(s) + 1);
	if (d) strcpy(d, s);
	return d;
}

int exr_crypto_attrs(const char *layer, const char *const *names, uint32_t count, struct exr_attr out[4]) {
	static const char *const what[4] = {"name", "hash", "conversion", "manifest"};
	char key[16];
	snprintf(key, sizeof(key), "%08x", exr_crypto_id(layer));
	key[7] = 0;          /* the first 7 hex digits */
	struct bytes m = {0};
	put(&m, "{", 1);
	for (uint32_t i = 0; i < count; ++i) {
		char hex[16];
		if (i) put(&m, ",", 1);
		put_json_string(&m, names[i]);
		snprintf(hex, sizeof(hex), ":\"%08x\"", exr_crypto_id(names[i]));
		put_str(&m, hex);
	}
	put(&m, "}", 2);          /* (with its terminator) */
	const char *value[4] = {layer, "MurmurHash3_32", "uint32_to_float32", m.failed ? NULL : (const char *)m.p};
	int rc = m.failed ? -1 : 0;
	for (int k = 0; k < 4; ++k) {
		char name[64];
		snprintf(name, sizeof(name), "cryptomatte/%s/%s", key, what[k]);
		out[k].name = dup_str(name);
		out[k].value = value[k] ? dup_str(value[k]) : NULL;
		if (!out[k].name || !out[k].value) rc = -1;
	}
	free(m.p);
	if (rc) exr_free_attrs(out, 4);
	return rc;
}

void exr_free_attrs(struct exr_attr *attrs, int count) {
	for (int k = 0; k < count; ++k) { free(attrs[k].name); free(attrs[k].value); attrs[k].name = attrs[k].value = NULL; }
}

struct named_channel { char name[EXR_MAX_NAME + 1]; crh_pack_channel ch; };
static int by_name(const void *a, const void *b) { return strcmp(((const struct named_channel *)a)->name, ((const struct named_channel *)b)->name); }

int exr_layer_channels(const float *fb, const float *aov, const float *denoised, const float *instance_ranked, const float *material_ranked,
                       const uint32_t *instance_map, uint32_t instance_count, const uint32_t *material_map, uint32_t material_count,
                       crh_pack_channel channels[CRH_PACK_MAX_CHANNELS], const char *names[CRH_PACK_MAX_CHANNELS]) {
	static struct named_channel list[CRH_PACK_MAX_CHANNELS];          /* (the names handed back live here: one caller at a time) */
	static const char *const rgb[3] = {"R", "G", "B"};
	static const char *const guides[CRH_AOV_CHANNELS] = {"albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "Z", "A"};
	int n = 0;
	memset(list, 0, sizeof(list));
	for (uint32_t i = 0; i < 3; ++i, ++n) { strcpy(list[n].name, rgb[i]); list[n].ch = (crh_pack_channel){fb, 3, i, NULL, 0, 0}; }
	for (uint32_t i = 0; aov && i < CRH_AOV_CHANNELS; ++i, ++n) { strcpy(list[n].name, guides[i]); list[n].ch = (crh_pack_channel){aov, CRH_AOV_CHANNELS, i, NULL, 0, 0}; }
	for (uint32_t i = 0; denoised && i < 3; ++i, ++n) { snprintf(list[n].name, sizeof(list[n].name), "denoised.%s", rgb[i]); list[n].ch = (crh_pack_channel){denoised, 3, i, NULL, 0, 0}; }
	for (int layer = 0; layer < 2; ++layer) {
		const float *ranked = layer ? material_ranked : instance_ranked;
		if (!ranked) continue;
		/* (id, coverage) of rank 2k in <layer>0k.R / .G, of rank 2k + 1 in .B / .A: component i of the twelve is channel "RGBA"[i % 4] of layer i / 4 */
		for (uint32_t i = 0; i < 2 * EXR_CRYPTO_RANKS; ++i, ++n) {
			snprintf(list[n].name, sizeof(list[n].name), "%s%02u.%c", layer ? "CryptoMaterial" : "CryptoObject", i / 4u, "RGBA"[i % 4u]);
			const int isId = i % 2u == 0;
			list[n].ch = (crh_pack_channel){ranked, 2 * EXR_CRYPTO_RANKS, i, isId ? (layer ? material_map : instance_map) : NULL, isId ? (layer ? material_count : instance_count) : 0, 0};
		}
	}
	qsort(list, (size_t)n, sizeof(list[0]), by_name);
	for (int i = 0; i < n; ++i) { channels[i] = list[i].ch; names[i] = list[i].name; }
	return n;
}

struct attr { const char *name, *type; const void *value; size_t size; };
static int attr_by_name(const void *a, const void *b) { return strcmp(((const struct attr *)a)->name, ((const struct attr *)b)->name); }

int exr_write_file(const char *path, int width, int height, const char *const *channel_names, const uint8_t *pixel_types, int channel_count, const struct exr_attr *strings,
                   int string_count, int compression, const void *chunk_data, const uint64_t *chunk_sizes, int chunk_count) {
	if (width <= 0 || height <= 0 || channel_count <= 0 || string_count < 0 || !chunk_data || !chunk_sizes) return -1;
	if (compression != 0 && compression != 2 && compression != 3) return -1;
	const int lines = compression == 3 ? 16 : 1;
	if (chunk_count != (height + lines - 1) / lines) return -1;
	for (int c = 0; pixel_types && c < channel_count; ++c) if (pixel_types[c] != EXR_FLOAT && pixel_types[c] != EXR_HALF) return -1;
	const unsigned char kind = (unsigned char)compression;
	struct bytes chlist = {0}, window = {0}, one = {0}, zero2 = {0}, head = {0};
	for (int c = 0; c < channel_count; ++c) {
		const size_t len = strlen(channel_names[c]);
		assert(len >= 1 && len <= EXR_MAX_NAME);
		if (len < 1 || len > EXR_MAX_NAME || (c && strcmp(channel_names[c - 1], channel_names[c]) >= 0)) { free(chlist.p); return -1; }
		put(&chlist, channel_names[c], len + 1);
		put_u32(&chlist, pixel_types && pixel_types[c] == EXR_HALF ? 1u : 2u);          /* HALF / FLOAT */
		put_u32(&chlist, 0u);          /* pLinear 0 and three zero bytes */
		put_u32(&chlist, 1u); put_u32(&chlist, 1u);
	}
	put(&chlist, "", 1);
	put_u32(&window, 0u); put_u32(&window, 0u); put_u32(&window, (uint32_t)(width - 1)); put_u32(&window, (uint32_t)(height - 1));
	put_u32(&one, 0x3f800000u);          /* 1.0f */
	put_u64(&zero2, 0u);                 /* 0.0f, 0.0f */
	const int count = 8 + string_count;
	struct attr *attrs = malloc((size_t)count * sizeof(*attrs));
	int rc = attrs && !chlist.failed && !window.failed && !one.failed && !zero2.failed ? 0 : -1;
	if (!rc) {
		attrs[0] = (struct attr){"channels", "chlist", chlist.p, chlist.n};
		attrs[1] = (struct attr){"compression", "compression", &kind, 1};
		attrs[2] = (struct attr){"dataWindow", "box2i", window.p, window.n};
		attrs[3] = (struct attr){"displayWindow", "box2i", window.p, window.n};
		attrs[4] = (struct attr){"lineOrder", "lineOrder", "", 1};
		attrs[5] = (struct attr){"pixelAspectRatio", "float", one.p, one.n};
		attrs[6] = (struct attr){"screenWindowCenter", "v2f", zero2.p, zero2.n};
		attrs[7] = (struct attr){"screenWindowWidth", "float", one.p, one.n};
		for (int k = 0; k < string_count; ++k) attrs[8 + k] = (struct attr){strings[k].name, "string", strings[k].value, strlen(strings[k].value)};
		qsort(attrs, (size_t)count, sizeof(*attrs), attr_by_name);
		static const unsigned char magic[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
		put(&head, magic, 8);
		for (int k = 0; k < count && !rc; ++k) {
			const size_t len = strlen(attrs[k].name);
			assert(len >= 1 && len <= EXR_MAX_NAME);
			if (len < 1 || len > EXR_MAX_NAME) rc = -1;
			put_attr(&head, attrs[k].name, attrs[k].type, attrs[k].value, attrs[k].size);
		}
		put(&head, "", 1);
		uint64_t at = head.n + 8u * (uint64_t)chunk_count, total = 0;
		for (int k = 0; k < chunk_count; ++k) {
			if (chunk_sizes[k] < 8u) rc = -1;
			put_u64(&head, at + total);
			total += chunk_sizes[k];
		}
		if (head.failed) rc = -1;
		FILE *f = rc ? NULL : fopen(path, "wb");
		if (!f) rc = -1;
		else {
			if (fwrite(head.p, 1, head.n, f) != head.n || fwrite(chunk_data, 1, (size_t)total, f) != (size_t)total) rc = -1;
			if (fclose(f) != 0) rc = -1;
		}
	}
	free(attrs); free(chlist.p); free(window.p); free(one.p); free(zero2.p); free(head.p);
	return rc;
}

int exr_half_types(const char *const *channel_names, int channel_count, uint8_t *pixel_types) {
	static const char *const set[12] = {"R", "G", "B", "albedo.R", "albedo.G", "albedo.B", "normal.X", "normal.Y", "normal.Z", "denoised.R", "denoised.G", "denoised.B"};
	int n = 0;
	for (int c = 0; c < channel_count; ++c) {
		pixel_types[c] = EXR_FLOAT;
		for (int k = 0; k < 12; ++k) if (!strcmp(channel_names[c], set[k])) { pixel_types[c] = EXR_HALF; ++n; }
	}
	return n;
}
