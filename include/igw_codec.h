/*
 * igw_codec.h -- C ABI of the frame codec (libigw_codec.so): baseline JPEG of rendered frames, on the device.
 *
 * The frames are what libigw_render.so writes (include/igw_render.h): uint8 [n][height][width][channels], row 0 the top
 * image row.  Each becomes one self-contained JFIF stream: baseline sequential DCT, 8 bit, YCbCr 4:4:4, one scan, the
 * Annex K quantisation tables scaled by `quality` with the IJG rule, the Annex K Huffman tables, no restart markers.
 * The arithmetic is integer and specified to the bit in DESIGN.md, section 9 ("JPEG frames and MJPEG video"), so the
 * bytes of a stream have exactly one right value; tests/jpeg_model.py is a numpy model of that section.
 *
 * Plain device pointers; the call is asynchronous on `stream` (hipStream_t as void*, NULL = default stream), never
 * allocates, never synchronises, and returns 0 or a negative igw_codec_status (igw_codec_last_error() gives the
 * message).  This library neither links nor knows the step and render libraries.
 */
#ifndef IGW_CODEC_H
#define IGW_CODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_CODEC_VERSION 1
#define IGW_CODEC_MAX_SIDE 1024       /* largest frame width / height (IGW_RENDER_MAX_SIDE) */
#define IGW_JPEG_HEADER_BYTES 623     /* SOI .. SOS of every stream: the same length at every size and quality */

enum igw_codec_status {
    IGW_CODEC_OK = 0,
    IGW_CODEC_ERR_INVALID = -1,   /* bad argument */
    IGW_CODEC_ERR_NO_DEVICE = -2, /* no usable HIP device (there is no CPU fallback) */
    IGW_CODEC_ERR_HIP = -3        /* a HIP call failed */
};

int igw_codec_version(void);
/* sha256 prefix of the codec's sources and flags (gridworld_amd/codec.py: source_hash) */
const char* igw_codec_build_id(void);
const char* igw_codec_last_error(void);

/*
 * A stride that holds the stream of any width x height frame at any quality: the header, 420 bytes for each of the
 * 3 * ceil(width / 8) * ceil(height / 8) blocks (a block's longest code sequence is 20 + 63 * 26 bits < 210 bytes, and
 * stuffing at most doubles it), and the end marker, rounded up to a multiple of 16.  0 for a size outside
 * 1..IGW_CODEC_MAX_SIDE.  Host arithmetic only: no device is needed.
 */
int64_t igw_jpeg_bound(int32_t width, int32_t height);

/*
 * Encodes n frames, one workgroup per frame, in one launch.
 *   frames  [n][height][width][channels] uint8, channels 3 (RGB) or 4 (RGBA: the fourth byte is ignored)
 *   quality 1..100
 *   out     [n][stride] bytes: stream i starts at out + i * stride
 *   stride  bytes per frame slot, >= IGW_JPEG_HEADER_BYTES + 2
 *   sizes   [n] int32 (4-byte aligned): the length of stream i.  If the stream does not fit in `stride`, sizes[i] is
 *           MINUS the length it needs, the slot holds the first `stride` bytes of it and nothing past the slot is
 *           written; igw_jpeg_bound() gives a stride that always fits.
 * Bytes of a slot between sizes[i] and stride are never written.  Offsets are 64-bit.  n == 0 is a no-op.  An invalid
 * argument (-1) is reported ahead of a missing device (-2).
 */
int igw_jpeg_encode(const uint8_t* frames, int64_t n, int32_t width, int32_t height, int32_t channels, int32_t quality,
                    uint8_t* out, int64_t stride, int32_t* sizes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
