/*
 * igw_render_obs.h -- C ABI of the training-layout observation of the first-person renderer (libigw_render_obs.so).
 *
 * An addition to version 1 of include/igw_render.h, in a library of its own: libigw_render.so and its build id stay
 * what they were, and this library compiles the same per-block ray caster (gridworld_amd/csrc/render/
 * igw_render_frame.h), so the frame it draws is igw_render_pov's, byte for byte.  Conventions (device pointers, the
 * stream, the status codes) are include/igw_render.h's.
 */
#ifndef IGW_RENDER_OBS_H_ABI
#define IGW_RENDER_OBS_H_ABI

#include "igw_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sha256 prefix of this library's sources and flags (gridworld_amd/render.py: OBS_LIBRARY.source_hash) */
const char* igw_render_obs_build_id(void);
const char* igw_render_obs_last_error(void);

/*
 * The observation a policy network reads, written by the launch that draws the frame: channel-first, optionally
 * reduced to luminance, converted to a float type with a scale and a bias, and stacked over the last K frames.
 * `data` is [n][stack][planes][height][width] elements of `dtype` (planes = gray ? 1 : 3; row 0 = top image row),
 * indexed with 64-bit offsets; seen as [n][stack * planes][height][width] it is the tensor a convolution takes.
 * For env i, pixel p, plane c, with (R, G, B) the bytes igw_render_pov draws for that pixel:
 *   v    = R, G, B for planes 0, 1, 2 (gray == 0), or the one luminance (19595 R + 38470 G + 7471 B + 32768) >> 16
 *          (gray == 1: the Y of the JPEG encoder, include/igw_codec.h);
 *   new  = v (IGW_OBS_U8); (float)v * scale, then + bias, two f32 operations that are never fused (IGW_OBS_F32);
 *          that f32 value rounded to nearest-even (IGW_OBS_F16, IGW_OBS_BF16).
 * Slot stack - 1 is the frame this launch draws, slot 0 the oldest.  If `fill` is set or env i restarts, every slot
 * of (i, c, p) becomes `new`; otherwise slot k takes the old slot k + 1 for k < stack - 1 and slot stack - 1 becomes
 * `new` (in place: `data` is the stack the previous launch left).  With stack == 1 `data` is never read.
 * Env i restarts iff `restart` is not NULL and restart[i * restart_stride] != 0: a device byte per env at any stride
 * in bytes, 64 for the `done` byte of the step path's output records (include/igw.h; after a step that ended an
 * episode of an auto-reset env the frame already shows the next episode), 1 for a mask.  It is read on the device only.
 * The struct itself is host memory, read during the call; its values reach the kernel by value.
 */
enum { IGW_OBS_U8 = 0, IGW_OBS_F16 = 1, IGW_OBS_BF16 = 2, IGW_OBS_F32 = 3 };
#define IGW_RENDER_HAS_OBS 1           /* igw_render_pov_obs and igw_render_obs exist (libigw_render_obs.so) */
#define IGW_RENDER_MAX_STACK 8        /* largest igw_render_obs.stack */
#define IGW_RENDER_OBS_BYTES 48       /* sizeof(igw_render_obs) */
typedef struct igw_render_obs {
    void*          data;            /* [n][stack][planes][height][width] elements of dtype; planes = gray ? 1 : 3 */
    int32_t        dtype;           /* IGW_OBS_* */
    int32_t        gray;            /* 0: planes R, G, B; 1: one luminance plane */
    int32_t        stack;           /* K, 1..8; slot 0 oldest, slot K-1 the frame this launch draws */
    int32_t        fill;            /* != 0: every env restarts its stack in this launch */
    float          scale, bias;     /* float dtypes; U8 requires scale == 1 and bias == 0 */
    const uint8_t* restart;         /* NULL, or env i restarts iff restart[i * restart_stride] != 0 */
    int64_t        restart_stride;  /* bytes; 64 for the `done` byte of the step path's output records, 1 for a mask */
} igw_render_obs;

/*
 * igw_render_pov with the observation of `obs` (not NULL): the arguments of the sibling without `channels`.  `out`
 * may be NULL (the observation alone); otherwise it receives the frame [n][height][width][3], byte-identical to
 * igw_render_pov(..., channels = 3).  IGW_RENDER_ERR_INVALID for the sibling's reasons and for a dtype that is not an
 * IGW_OBS_*, a stack outside 1..IGW_RENDER_MAX_STACK, a scale or bias that is not finite, IGW_OBS_U8 with scale != 1
 * or bias != 0, a NULL `data` (n > 0), a `data` not aligned to its element size, and a restart_stride < 1 with a
 * `restart`.  Nothing outside data[0 .. n * stack * planes * height * width) and `out` is written.  n == 0 is a
 * no-op; asynchronous on `stream`, never allocates, never synchronises, like the sibling.  Returns 0 or a negative
 * igw_render_status; igw_render_obs_last_error() gives the message.
 */
int igw_render_pov_obs(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                       int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, const igw_render_obs* obs,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
