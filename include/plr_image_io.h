/* DDS reader / writer of the reference's asset pipeline: the on-disk format of baked SDF volumes.
 *
 * Replaces  bool loadDDSFile(const std::filesystem::path&, ImageDescription*, std::vector<uint8_t>*)   (Common/ImageIO.cpp:342-431)
 *      and  void writeDDSFile(const std::filesystem::path&, const ImageDescription&, const std::vector<uint8_t>&)   (ImageIO.cpp:448-571).
 * File layout: magic 0x20534444 ("DDS "), the 124-byte DDS_header, for fourCC "DX10" the 20-byte DDS_headerDX10, then the raw texels
 * (x fastest, then y, then z; all mips consecutively). The writer emits a DX10 header for the formats RGBA8 and R16_sFloat, as the
 * reference, and - beyond the reference - a legacy header with the fourCC DXT1 / DXT5 / ATI2 for a BC1 / BC3 / BC5 payload (the blocks
 * plr_encode_rgba8_to_bc makes), which the reader takes back; the reader understands DX10/R16_FLOAT and the legacy fourCCs DXT1 (BC1), DXT5 (BC3), ATI2 (BC5), as the reference.
 * plr_decode_bc_to_rgba8 decodes the blocks of such a file's BC1 / BC3 / BC5 levels on the host.
 * All functions return PLR_OK (0) or a negative code; plr_last_error() (plr.h) explains. No GPU is involved. */
#ifndef PLR_IMAGE_IO_H
#define PLR_IMAGE_IO_H
#include "plr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* writeDDSFile. data_size must be a multiple of 4 (the reference copies whole dwords, ImageIO.cpp:557-569). */
int plr_write_dds_file(const char* path, const plr_image_desc* desc, const void* data, size_t data_size);

/* loadDDSFile. Fills out_desc (type from height/depth, mipCount = Manual with the file's mip count, usage Sampled). The texel
 * payload (file size minus headers) is returned in *out_data_size; it is copied to out_data when out_data is non-null and
 * capacity suffices (call once with out_data = NULL to size the buffer). */
int plr_load_dds_file(const char* path, plr_image_desc* out_desc, void* out_data, size_t capacity, size_t* out_data_size);

/* in-memory forms of the same (used by the file functions): serialise to / parse from a byte buffer */
int plr_encode_dds(const plr_image_desc* desc, const void* data, size_t data_size, void* out_file, size_t capacity, size_t* out_file_size);
int plr_decode_dds(const void* file, size_t file_size, plr_image_desc* out_desc, size_t* out_data_offset, size_t* out_data_size);

/* One level of a block-compressed image to RGBA8 words, R in the low byte, in plain integer arithmetic: the decode "depthPrepassRaster.comp" applies to the taps of a
 * compressed scene texture (DESIGN.md "Block-compressed textures in the depth prepass"), so a caller can hand the same codes to an entry point that takes RGBA8
 * only (plrf_set_shadow_caster_cutouts). format: PLR_FORMAT_BC1 (8-byte blocks: (r, g, b, 255), three-colour mode with an opaque black index 3 where c0 <= c1),
 * PLR_FORMAT_BC3 (16-byte blocks: alpha block, then a colour block that is always in four-colour mode) or PLR_FORMAT_BC5 (16-byte blocks: (R, G, 0, 255)). The
 * level is ceil(width / 4) x ceil(height / 4) blocks, row-major; texel (x, y) is position 4 (y & 3) + (x & 3) of block (x >> 2, y >> 2). bytes must be exactly
 * the level's size; out_words receives width * height words. PLR_ERR_INVALID_ARGUMENT: another format, a side of 0 or above 16384, a NULL pointer, a byte count
 * other than the level's. */
int plr_decode_bc_to_rgba8(int format, uint32_t width, uint32_t height, const void* blocks, uint64_t bytes, uint32_t* out_words);

/* The twin of the decode: one level of width * height RGBA8 words into its BC1 / BC3 / BC5 blocks by the encode contract "textureBlockEncode.comp" applies
 * (DESIGN.md "Texture store built on the GPU": range fit in integers - block (bx, by) gathers texel (min(4 bx + i, W - 1), min(4 by + j, H - 1)) at position
 * 4 j + i; BC1 and BC3's colour block take r, g, b, BC3's alpha block a, BC5's two blocks r and g). The same bytes as the GPU pass writes, without a GPU: a
 * caller can encode the cutouts it decodes for plrf_set_shadow_caster_cutouts, or write a compressed DDS file. bytes must be exactly the level's size, which
 * out_blocks receives. PLR_ERR_INVALID_ARGUMENT: what the decode refuses. */
int plr_encode_rgba8_to_bc(int format, uint32_t width, uint32_t height, const uint32_t* words, void* out_blocks, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
