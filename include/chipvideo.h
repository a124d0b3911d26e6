/*
 * chipvideo.h — C ABI of CHIPVideo, the MI355X (gfx950) compute backend for
 * SwiftVideo's picture path.
 *
 * This header is what a SwiftPM system-library target `CHIPVideo` exposes to
 * `compute.hip.swift` (the way Sources/CCUDA/module.modulemap:1-6 exposes
 * cuda.h to compute.cuda.swift).  Every entry point names the reference
 * interface it replaces; citations are into unpause-live/SwiftVideo,
 * `Sources/SwiftVideo/` unless a directory is given.
 *
 * Conventions
 *  - plain C, no C++/torch types; every function returns a chv_status
 *    (0 = success), never aborts, never throws across the boundary
 *    (errors surface in Swift as `ComputeError`, compute.swift:22-39);
 *  - a chv_context is used by one thread at a time; different contexts on the
 *    same device may be entered concurrently (GPUBarrierUpload/Download run on
 *    Bus runner threads with their own shared context, compute.swift:177,234);
 *  - chv_buffer_free may be called from any thread at any time
 *    (ComputeBuffer.deinit, compute.cl.swift:55-57);
 *  - pixel work only ever runs on the GPU: there is no CPU fallback and a
 *    missing/unsupported device is an error, not a slow path.
 */
#ifndef CHIPVIDEO_H
#define CHIPVIDEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHV_VERSION 0x000100

/* ---- status codes: one per ComputeError case, compute.swift:22-39 -------- */
typedef enum chv_status {
    CHV_OK = 0,
    CHV_ERR_INVALID_VALUE = 1,        /* .invalidValue                       */
    CHV_ERR_OUT_OF_MEMORY = 2,        /* .outOfMemory                        */
    CHV_ERR_INVALID_CONTEXT = 3,      /* .invalidContext                     */
    CHV_ERR_BAD_TARGET = 4,           /* .badTarget                          */
    CHV_ERR_BAD_INPUT = 5,            /* .badInputData                       */
    CHV_ERR_NOT_IMPLEMENTED = 6,      /* .notImplemented                     */
    CHV_ERR_KERNEL_NOT_FOUND = 7,     /* .computeKernelNotFound              */
    CHV_ERR_DEVICE_NOT_AVAILABLE = 8, /* .deviceNotAvailable                 */
    CHV_ERR_INVALID_DEVICE = 9,       /* .invalidDevice                      */
    CHV_ERR_INVALID_OPERATION = 10,   /* .invalidOperation                   */
    CHV_ERR_BAD_CONTEXT_STATE = 11,   /* .badContextState                    */
    CHV_ERR_INVALID_PLATFORM = 12,    /* .invalidPlatform                    */
    CHV_ERR_UNKNOWN = 13              /* .unknownError                       */
} chv_status;

/* Static string for a status (the checkCLError/check() tables,
 * compute.cl.swift:683-702, compute.cuda.swift:102-112). */
const char *chv_error_string(int status);
/* Thread-local detail text of the last failing call on this thread ("" if none). */
const char *chv_last_error_detail(void);
int chv_version(void);
/* What the library was built with: "arch=<the Makefile's ARCH>;hipcc=<HIP version>;clang=<major.minor>;fp_contract=off;tick_bgra_wave:abl=0,...;
 * ...;lanczos3:abl=0".  `abl` != 0 marks a timing-only ablation build whose pixels are wrong by design (profiles/r02_notes.md section 6):
 * tests/test_abi.py asserts 0 for every kernel family, bench.py prints the string.  The compiler version is there because the streaming and
 * Lanczos strip kernels are scheduled by hand against one hipcc (tests/test_device_code_contract.py pins major.minor). */
const char *chv_build_flags(void);
/* Measurement / test hook: path-selection switches.  Names and values are those of the environment variables read once at
 * first use (CHV_FORCE_GENERAL=1, CHV_BGRA_PATH=wave|tiled|stream, CHV_WAVE_ROWS=8|16, CHV_TILE_ROWS=16|32, CHV_SAME_GEOM=0,
 * CHV_DESC=host|device, CHV_STREAM=0, CHV_YUV_STREAM=0|force, CHV_WAVE_DMA=0, CHV_PASS_FUSE=0, CHV_GEOM_CACHE=0|eager, CHV_STREAM_ROWS=n,
 * CHV_STREAM_OPAQUE=0, CHV_STREAM_CARRY=0, CHV_REBIND=scatter|copy);
 * NULL or "" restores the default.  Process-wide, atomic; not part of the Swift-facing contract. */
int chv_debug_set_switch(const char *name, const char *value);
/* Measurement / test hook: counters of the current device's store of strip-kernel geometry tables (csrc/geom_cache.h): "geom_store_patched"
 * (launches whose layers were pointed at stored tables before their descriptors travelled: batches at creation, lone ticks),
 * "geom_store_batch_hits", "geom_store_builds", "geom_store_bytes", "geom_store_tables"; and "stream_opaque_launches", the launches of
 * tick_bgra_stream that took the opaque-bottom kernels, and "stream_carry_launches", those of them that took the chroma-carry kernels, "stream_f32tap_launches", those of these that took the f32-tap kernels, and "stream_phased_launches", the launches of tick_bgra_stream cut into more than one phase (csrc/stream_plan.h),
 * (process-wide); and "lanczos_ladder_launches", the device launches made by chv_scale_lanczos_to_yuv_ladder (process-wide: one per chunk for a
 * ladder whose rungs all take one route, two for one with rungs on both), and "lanczos_planar_ladder_launches", the same count for
 * chv_scale_lanczos_ladder (process-wide), and "lanczos_420_ladder_launches", the same count for the cross-format path (NV12 -> y420p,
 * y420p -> NV12) of chv_scale_lanczos_420 and chv_scale_lanczos_420_ladder (process-wide; same-format pairs through those entries are forwarded
 * and counted by "lanczos_planar_ladder_launches" or not at all, like the calls they forward to), and "lanczos_to_420_launches", the same count for
 * the five formats chv_scale_lanczos_to_420 and chv_scale_lanczos_to_420_ladder do not forward (process-wide), and "lanczos_hbd_launches", the same
 * count for chv_scale_lanczos_hbd_to_420 and chv_scale_lanczos_hbd_to_420_ladder (process-wide), and "lanczos_from_yuv_launches", the device
 * launches made by chv_scale_lanczos_from_yuv and chv_scale_lanczos_from_yuv_batch (process-wide: one per call, one per chunk), and
 * "lanczos_from_yuv_ladder_launches", the device launches made by chv_scale_lanczos_from_yuv_ladder (process-wide: one per chunk for a ladder
 * whose rungs all take one route, two for one with rungs on both; that entry does not touch "lanczos_from_yuv_launches"), and
 * "lanczos_rgb_ladder_launches", the same count for chv_scale_lanczos_rgb_ladder (process-wide; that entry touches no other counter).
 * Unknown name -> CHV_ERR_INVALID_VALUE. */
int chv_debug_get_counter(const char *name, unsigned long long *value);

/* ---- kernels: `enum ComputeKernel`, compute.swift:49-74 ------------------ */
typedef enum chv_kernel {
    CHV_K_IMG_NV12_NV12 = 0,
    CHV_K_IMG_BGRA_NV12 = 1,
    CHV_K_IMG_RGBA_NV12 = 2,
    CHV_K_IMG_BGRA_BGRA = 3,    /* semantics of kernels.metal:52-62 */
    CHV_K_IMG_Y420P_Y420P = 4,
    CHV_K_IMG_Y420P_NV12 = 5,
    CHV_K_IMG_CLEAR_NV12 = 6,
    CHV_K_IMG_CLEAR_YUVS = 7,   /* enum case without a kernel in any backend */
    CHV_K_IMG_CLEAR_BGRA = 8,
    CHV_K_IMG_CLEAR_Y420P = 9,
    CHV_K_IMG_CLEAR_RGBA = 10,  /* name resolves to CLEAR_BGRA, compute.swift:101 */
    CHV_K_IMG_RGBA_Y420P = 11,
    CHV_K_IMG_BGRA_Y420P = 12,
    CHV_K_SND_S16I_S16I = 13,   /* audio mix; chv_snd_uniforms below */
    CHV_K_ME_FULLSEARCH = 14,   /* block motion search; chv_me_uniforms below */
    /* Kernels VideoMixer.findKernel can name (mix.video.swift:142-146) but no
     * reference backend implements; specification in DESIGN.md section 4. */
    CHV_K_IMG_NV12_BGRA = 32,
    CHV_K_IMG_Y420P_BGRA = 33,
    CHV_K_IMG_BGRA_BGRA_TX = 34, /* transform/opacity/fill-aware BGRA over BGRA */
    CHV_K_IMG_RGBA_BGRA_TX = 35,
    /* The encoder side of "integer BT.601/709 YUV <-> RGB": an RGB picture onto a 4:2:0 canvas through the 16.16 integer
     * matrix of chv_kernel_opts.colorspace (the reference's img_bgra_nv12 family is a float full-range matrix with a 0.113
     * blue weight, kernels.cl.swift:96-99).  Specification in DESIGN.md section 4.5. */
    CHV_K_IMG_BGRA_NV12_INT = 36,
    CHV_K_IMG_RGBA_NV12_INT = 37,
    CHV_K_IMG_BGRA_Y420P_INT = 38,
    CHV_K_IMG_RGBA_Y420P_INT = 39
} chv_kernel;

/* defaultComputeKernelFromString, compute.swift:90-110, plus the entries of the
 * compute.swift hunk in INTEGRATION.md section 1: the eight names above and
 * "img_rgba_bgra" (-> CHV_K_IMG_RGBA_BGRA_TX; what VideoMixer.findKernel,
 * mix.video.swift:142-146, synthesises for an RGBA layer on a BGRA canvas).
 * Unknown name -> CHV_ERR_INVALID_VALUE, as the reference throws. */
int chv_kernel_from_string(const char *name, int *kernel);
/* String(describing: ComputeKernel) — the round trip computeTests.swift:9-39 checks. */
const char *chv_kernel_name(int kernel);

/* ---- pixel formats: `enum PixelFormat`, sample.pict.swift:20-33 ---------- */
typedef enum chv_pixel_format {
    CHV_FMT_NV12 = 0, CHV_FMT_NV21 = 1, CHV_FMT_YUVS = 2, CHV_FMT_ZVUY = 3,
    CHV_FMT_Y420P = 4, CHV_FMT_Y422P = 5, CHV_FMT_Y444P = 6,
    CHV_FMT_RGBA = 7, CHV_FMT_BGRA = 8, CHV_FMT_INVALID = 11,
    /* 10-bit 4:2:0 (no reference counterpart: sample.pict.swift:19 leaves them open).  Sources of chv_scale_lanczos_hbd_to_420 only; every other
     * entry treats them as any unknown format.  chv_plane.components is the BYTES of a texel. */
    CHV_FMT_P010 = 12,      /* 2 planes: Y (components 2), CbCr (components 4); code = little-endian word >> 6 */
    CHV_FMT_Y420P10 = 13    /* 3 planes of components 2: Y, Cb, Cr (FFmpeg's yuv420p10le); code = word & 1023 */
} chv_pixel_format;

/* Integer YUV->RGB matrices for CHV_K_IMG_{NV12,Y420P}_BGRA. */
typedef enum chv_colorspace {
    CHV_CSC_BT601_LIMITED = 0, CHV_CSC_BT709_LIMITED = 1,
    CHV_CSC_BT601_FULL = 2, CHV_CSC_BT709_FULL = 3
} chv_colorspace;

/* ---- devices: ComputeDevice / availableComputeDevices,
 *      compute.cl.swift:36-44,107-109 ----------------------------------- */
typedef struct chv_device_info {
    int32_t index;
    int32_t available;        /* ComputeDevice.available  */
    int32_t device_type;      /* 0 = GPU (ComputeDeviceType, compute.swift:41-46) */
    int32_t vendor_id;        /* PCI vendor, 0x1002       */
    int32_t compute_units;
    int32_t supports_images;  /* 0: gfx950 has no image path; planes are linear */
    uint64_t total_memory;
    char name[128];
    char arch[32];            /* "gfx950..." */
} chv_device_info;

int chv_device_count(int *count);
int chv_device_info_get(int device, chv_device_info *info);

/* ---- contexts: ComputeContext, compute.cl.swift:75-105 ------------------ */
typedef struct chv_context chv_context;

/* createComputeContext(_:logger:), compute.cl.swift:115-145.  One HIP stream
 * per context; all kernels are part of the library (no per-context build). */
int chv_context_create(int device, chv_context **out);
/* createComputeContext(sharing:), compute.cl.swift:111-113: same device and
 * allocator, a NEW stream (the reference makes a new command queue, :82-87). */
int chv_context_share(chv_context *parent, chv_context **out);
/* destroyComputeContext, compute.cl.swift:147-151 */
int chv_context_destroy(chv_context *ctx);
int chv_context_device(chv_context *ctx, int *device);
/* Raw hipStream_t of the context, for callers that interleave their own work. */
int chv_context_stream(chv_context *ctx, void **hip_stream);
/* NUMA node of the device's PCIe root complex (sysfs), -1 if unknown: where a host should pin its upload ring. */
int chv_context_numa_node(chv_context *ctx, int *node);

/* ---- device memory: ComputeBuffer, compute.cl.swift:46-58 ---------------- */
typedef struct chv_buffer chv_buffer;

/* createBuffer, compute.cl.swift:522-529 */
int chv_buffer_alloc(chv_context *ctx, size_t bytes, chv_buffer **out);
/* Adopt device memory owned by someone else (e.g. a decoder surface); never freed here. */
int chv_buffer_wrap(chv_context *ctx, void *device_ptr, size_t bytes, chv_buffer **out);
/* ComputeBuffer.deinit, compute.cl.swift:55-57; callable from any thread.  A buffer that kernels of a pass in progress name (chv_pass_begin)
 * is released when they have been launched; the call returns at once either way.  A second free of the same buffer is CHV_ERR_INVALID_VALUE
 * while the first is pending, undefined afterwards (as for any freed handle). */
int chv_buffer_free(chv_buffer *buf);
int chv_buffer_info(chv_buffer *buf, void **device_ptr, size_t *bytes);
/* One plane of createTexture (compute.cl.swift:532-581): `components` bytes
 * per texel (1 = R8, 2 = RG8, 4 = RGBA8).  Linear, pitch is 128-byte (cache line) aligned. */
int chv_plane_alloc(chv_context *ctx, int width, int height, int components,
                    chv_buffer **out, size_t *pitch);

/* uploadComputeBuffer / the per-plane clEnqueueWriteImage of
 * uploadComputePicture (compute.cl.swift:361-379, 434-452): pitched H2D copy.
 * async = 0: returns when the copy is complete (reference behaviour).
 * async = 1: the host bytes are staged into pinned memory before returning, so
 *            `src` is only borrowed for the call; the copy is ordered on the
 *            context's stream.
 * async = 2: `src` is pinned memory from chv_host_alloc that the caller leaves
 *            unchanged until the context's stream has passed the copy (e.g. the
 *            next chv_pass_end(wait)); no staging copy is made — the path for
 *            decoders that write straight into pinned frames.
 * After an asynchronous upload, kernels launched from ANY context of the device
 * that read the plane wait for the copy on their own stream (an event per
 * buffer); no host-side wait is needed between upload and use. */
int chv_upload(chv_context *ctx, chv_buffer *dst, size_t dst_offset, size_t dst_pitch,
               const void *src, size_t src_pitch, size_t width_bytes, size_t rows, int async);
/* Pinned (page-locked) host memory for async = 2 uploads. */
int chv_host_alloc(chv_context *ctx, size_t bytes, void **out);
int chv_host_free(chv_context *ctx, void *ptr);

/* downloadComputeBuffer / downloadComputePicture (compute.cl.swift:381-396,
 * 461-498): pitched D2H copy, always complete on return. */
int chv_download(chv_context *ctx, void *dst, size_t dst_pitch, chv_buffer *src,
                 size_t src_offset, size_t src_pitch, size_t width_bytes, size_t rows);
/* The same copy without the wait (the D2H half of GPUBarrierDownload running on a context of its own, compute.swift:217-255, so that
 * the read-back of tick t overlaps the kernels of tick t + 1): ordered on ctx's stream behind pending asynchronous uploads of `src`;
 * `dst` is pinned memory from chv_host_alloc and holds the picture once ctx's stream has passed the copy (chv_event_record +
 * chv_event_synchronize, or chv_pass_end(ctx, wait)).  Kernels of ANOTHER context that write `src` are ordered in front of the copy
 * with chv_event_record (there) + chv_event_wait (here).  Adjacent planes / frames of one allocation travel as one linear copy when
 * both pitches equal width_bytes. */
int chv_download_async(chv_context *ctx, void *dst, size_t dst_pitch, chv_buffer *src,
                       size_t src_offset, size_t src_pitch, size_t width_bytes, size_t rows);

/* ---- images: POD view of ImageBuffer.planes + computeTextures,
 *      sample.pict.linux.swift:23-72 ------------------------------------- */
typedef struct chv_plane {
    chv_buffer *buffer;
    size_t offset;        /* bytes from the start of `buffer` */
    int32_t width, height;/* texels (Plane.size)  */
    int32_t pitch;        /* bytes  (Plane.stride) */
    int32_t components;   /* Plane.components.count */
} chv_plane;

typedef struct chv_image {
    int32_t format;       /* chv_pixel_format */
    int32_t width, height;
    int32_t n_planes;
    chv_plane planes[3];
} chv_image;

/* ImageUniforms, compute.swift:76-86: 236 bytes, no padding.  Each matrix is
 * M.inverse.transpose as uploaded by applyComputeImage (compute.swift:149-161),
 * i.e. floats [4i..4i+3] are what the kernels dot with to get component i. */
typedef struct chv_uniforms {
    float transform[16];
    float texture_transform[16];
    float border_matrix[16];
    float fill_color[4];
    float input_size[2];
    float output_size[2];
    float opacity;
    float image_time;
    float target_time;
} chv_uniforms;

typedef struct chv_kernel_opts {
    int32_t colorspace;   /* chv_colorspace; YUV->BGRA kernels only */
    int32_t reserved[3];
} chv_kernel_opts;

/* Uniforms of the two kernels of `enum ComputeKernel` no caller of the reference dispatches (compute.swift:67,70); both run through
 * chv_run_kernel in the reference's bind order [outputs][inputs][uniforms] (compute.cl.swift:288-327):
 *   CHV_K_SND_S16I_S16I (kernels.cl.swift:534-562)  target: ONE plane of 2-byte texels = interleaved-stereo int16 samples (width x height
 *       samples; rows contiguous when height > 1), updated in place (out[gid] += ...); inputs: inputCount..8 images of the same shape;
 *       uniforms: the 100-byte chv_snd_uniforms.  A float product below -32768 wraps as on the CPU the kernel string was compiled for
 *       (OpenCL leaves it undefined; oracle/ref_kernels.c::snd_cvt).
 *   CHV_K_ME_FULLSEARCH (kernels.metal:129-267)  target: one RGBA8 texel per block, (mv.x, 0.5, mv.y, 1) normalised to [0, 1]; inputs[0] =
 *       reference picture, inputs[1] = current picture (plane 0 of each, 1-component: the luma plane of an NV12 / y420p picture);
 *       uniforms: the 24-byte chv_me_uniforms, blockSize 1..64.  Bit-for-bit the Metal source, its sliding-window SAD included. */
typedef struct chv_snd_uniforms {     /* BufferUniforms, kernels.cl.swift:536-541 */
    int32_t input_count;
    int32_t input_offsets[8];         /* (not read by the kernel) */
    float input_gains[8];
    float input_fade[8];
} chv_snd_uniforms;
typedef struct chv_me_uniforms {      /* MotionEstimationUniforms, kernels.metal:33-37 */
    int32_t block_size[2];
    int32_t search_window_size[2];
    int32_t image_size[2];
} chv_me_uniforms;

/* ---- compute passes ----------------------------------------------------- */
/* beginComputePass, compute.cl.swift:234-237.
 * Between chv_pass_begin and chv_pass_end the picture kernels issued through chv_run_kernel are ACCEPTED — every argument check runs in the
 * call and its error comes back from it — and HELD: nothing has to be visible before the pass ends (usingContext, compute.swift:131-134), so
 * `img_clear_* + N layer kernels on one target`, what an unchanged VideoMixer issues per tick (mix.video.swift:116-124), leaves as the ONE
 * launch chv_composite would have made of it: same bytes (that equality is chv_composite's definition), one launch instead of N + 1.  What is
 * held goes out, in issue order, at chv_pass_end — or before anything else that touches ctx's stream: an upload or download through ctx, a
 * batch, a custom or buffer kernel, an event, chv_context_stream, a kernel on another target, a clear after layers, a layer whose
 * input shares device memory with the held target (compared by the planes' address ranges: the target itself, another handle wrapped over its
 * memory, a view of it with plane offsets — such a layer samples what the kernels issued before it wrote).  Buffers named by held
 * kernels may be passed to chv_buffer_free before the pass ends (a ComputeBuffer's deinit can run as soon as runComputeKernel returns,
 * compute.cl.swift:55-57): the free takes effect once they have been launched.  Work of OTHER contexts is ordered against a pass's kernels at the
 * pass's end, as against any kernel: events, or the per-buffer upload events.  Brackets nest (uploadComputePicture opens its own around its
 * copies, compute.cl.swift:433,453): kernels are held while any bracket is open, and every chv_pass_end launches what is held.  CHV_PASS_FUSE=0 (environment / chv_debug_set_switch) launches
 * every kernel in its call, as rounds 1-5 did. */
int chv_pass_begin(chv_context *ctx);
/* runComputeKernel (both overloads), compute.cl.swift:250-344.  Launch domain
 * is the target's plane-0 size (:329).  `inputs`/`n_inputs`: the images array;
 * `uniforms`/`uniforms_size`: the Swift struct bytes (236 for ImageUniforms,
 * 0/NULL for none); `blends`: bind the target again as the read-only current
 * image (:301-313).  `opts` may be NULL. */
int chv_run_kernel(chv_context *ctx, int kernel, const chv_image *target,
                   const chv_image *inputs, int n_inputs,
                   const void *uniforms, size_t uniforms_size, int blends,
                   const chv_kernel_opts *opts);
/* endComputePass, compute.cl.swift:346-359: launches what the pass holds (above; a launch error of those kernels is returned here), then
 * wait != 0 -> block until the stream is idle (clFinish), else just make sure work is submitted (clFlush). */
int chv_pass_end(chv_context *ctx, int wait);

/* ---- one mixer tick in one launch --------------------------------------- */
/* What VideoMixer.mix does per tick (mix.video.swift:116-124): clear the
 * backing image, then applyComputeImage for each layer in z order.
 * chv_composite produces byte-identical output to that sequence of
 * chv_run_kernel calls, but reads every layer once and writes the canvas once. */
typedef struct chv_layer {
    int32_t kernel;               /* img_<fmt>_<target fmt> */
    chv_image image;
    chv_uniforms uniforms;
    chv_kernel_opts opts;
} chv_layer;

/* Layers per launch of chv_composite; a deeper tick is issued as several launches
 * on the context's stream (same bytes: the canvas is 8-bit between layers anyway).
 * Ticks of a batch (chv_batch_create) may have any number of layers. */
#define CHV_MAX_LAYERS 16

int chv_composite(chv_context *ctx, const chv_image *target, int clear_first,
                  const chv_layer *layers, int n_layers);

/* Many independent ticks (streams / frames) in one launch: job i composites
 * layers[first_layer[i] .. first_layer[i]+n_layers[i]) onto targets[i].
 * A batch can be run any number of times; its scene (kernels, uniforms, geometry) is fixed at
 * creation, the pictures it is bound to can be exchanged with chv_batch_rebind below. */
typedef struct chv_batch chv_batch;
typedef struct chv_tick {
    chv_image target;
    int32_t clear_first;
    int32_t n_layers;
    const chv_layer *layers;
} chv_tick;
int chv_batch_create(chv_context *ctx, const chv_tick *ticks, int n_ticks, chv_batch **out);
int chv_batch_run(chv_context *ctx, chv_batch *batch);
int chv_batch_destroy(chv_batch *batch);
/* Point an existing batch at new pictures.  No reference counterpart: the reference issues every tick's kernels afresh.  What makes it worth
 * having is that a real host never shows the same pictures twice — the upload ring and VideoMixer.getBacking's ring of 10 canvases
 * (mix.video.swift:148-165) rotate every tick — while between two ticks of a scene nothing but plane addresses changes: rebinding and running
 * replaces chv_batch_create + run + destroy per group tick.
 *  - Same geometry, new memory.  A replacement must equal the picture it replaces in format, image size and plane count and, per used
 *    plane, in width, height, components AND pitch (the route, LF_SAME_GEOM and the launch geometry were derived from them); on every route but
 *    the general kernels its plane addresses must have the alignment the replaced ones had (modulo 16: multiples of 16 stay multiples of 16),
 *    4-component planes need 4 everywhere.  Every check chv_batch_create makes of a plane applies (buffer valid and on the batch's device,
 *    extent inside the buffer).  Anything else is CHV_ERR_INVALID_VALUE — or the BAD_INPUT / BAD_TARGET chv_batch_create gives for that plane —
 *    and the detail text says to rebuild the batch.  Views at any offset inside larger parents are fine as long as these hold.
 *  - All or nothing.  Every item is validated before anything changes; after an error (a failed enqueue included) the batch runs exactly as
 *    before the call.  The same slot named twice in one call is CHV_ERR_INVALID_VALUE.
 *  - Stream-ordered on ctx's stream like a run (a held pass goes out first): runs issued before the call composite the old pictures, runs
 *    issued after it, from any context of the device, the new ones; no host wait is needed between rebind, run, rebind, run, and in the steady
 *    state rebind -> run -> chv_pass_end(wait) the call never blocks the host.
 *  - Dependencies follow the pictures: later runs wait for pending asynchronous uploads of the buffers bound NOW and never touch a buffer that
 *    was rebound away, which may be freed once the runs issued before the rebind have completed.
 *  - chv_batch_describe, the route, a split into two launches and the geometry tables are untouched.  Changing uniforms, opacity or geometry
 *    is a new batch.
 * CHV_REBIND=scatter|copy picks the mechanism (a small kernel that stores the new addresses / the whole descriptor block again); default: the
 * library decides. */
typedef struct chv_rebind {
    int32_t tick;     /* index of the tick as given to chv_batch_create */
    int32_t layer;    /* -1: the tick's target; 0..n_layers-1: that layer's image, position within the tick as given to
                         chv_batch_create (also for batches that were split into two launches or have > 16 layers) */
    chv_image image;  /* the picture that takes the slot's place */
} chv_rebind;
int chv_batch_rebind(chv_context *ctx, chv_batch *batch, const chv_rebind *items, int n_items);
/* Name of the device kernel a batch dispatches to and its launch count (for profiling).  A batch whose ticks start with 2..4
 * full-frame videos of one geometry and go on with other layers runs as TWO launches on the context's stream ("tick_bgra_stream +
 * tick_bgra_wave": the videos, then the rest continuing on the canvas); the bytes are those of one pass. */
int chv_batch_describe(chv_batch *batch, char *kernel_name, size_t cap, int *n_launches);

/* ---- custom kernels ------------------------------------------------------ */
/* `ComputeKernel.custom(name:)` + buildComputeKernel (compute.swift:72-73,
 * compute.cl.swift:153-195, getComputeKernel :218-232): user source compiled at
 * run time and kept in the context's library under `name`.  Here the source
 * is HIP C++ compiled with hipRTC for the context's device; it is prefixed
 * with chv_custom_prelude() (the counterpart of kOpenCLKernelMatrixFuncs,
 * kernels.cl.swift:25-35, plus the image builtins OpenCL gives a kernel for
 * free) and must define
 *     extern "C" __global__ void <name>(chv_custom_args a)
 * The argument block carries what the reference binds positionally
 * (compute.cl.swift:288-335): the target planes, the same planes again as
 * `current` when `blends` (n_planes = 0 otherwise), the input images, the
 * uniforms' bytes.  Launch domain: one thread per texel of target plane 0 in
 * 16x16 blocks, rounded up — kernels test their coordinates (CHV_GUARD). */
#define CHV_CUSTOM_MAX_INPUTS 4
#define CHV_CUSTOM_MAX_UNIFORMS 256
typedef struct chv_dev_plane {
    uint8_t *ptr;                     /* device address of texel (0, 0) */
    int32_t width, height, pitch, components;
} chv_dev_plane;
typedef struct chv_dev_image {
    chv_dev_plane planes[3];
    int32_t n_planes, format;
} chv_dev_image;
typedef struct chv_custom_args {
    chv_dev_image target, current;
    chv_dev_image inputs[CHV_CUSTOM_MAX_INPUTS];
    int32_t n_inputs, uniforms_size;
    uint8_t uniforms[CHV_CUSTOM_MAX_UNIFORMS];
} chv_custom_args;
/* The text every custom source is prefixed with (struct definitions above, vecmat4, unorm8 load/store,
 * nearest and linear samplers with the semantics of the built-in kernels). */
const char *chv_custom_prelude(void);
/* buildComputeKernel.  Replaces an earlier kernel of the same name in this context's library; contexts made
 * with chv_context_share afterwards inherit the library.  Compile or lookup failure:
 * CHV_ERR_BAD_INPUT ("Unable to create kernel named ..."), build log in chv_last_error_detail(). */
int chv_kernel_build(chv_context *ctx, const char *name, const char *source);
/* runComputeKernel(kernel: .custom(name)).  CHV_ERR_KERNEL_NOT_FOUND if `name` is not in the library;
 * at most CHV_CUSTOM_MAX_INPUTS images and CHV_CUSTOM_MAX_UNIFORMS uniform bytes. */
int chv_run_custom(chv_context *ctx, const char *name, const chv_image *target,
                   const chv_image *inputs, int n_inputs,
                   const void *uniforms, size_t uniforms_size, int blends);

/* ---- resampling --------------------------------------------------------- */
/* Separable Lanczos-3 resize of `src` to the size of `dst`, no format conversion.  No reference counterpart; DESIGN.md section 4.4.
 * Three families, selected by `dst`:
 *   - one 4-component plane (BGRA or RGBA);
 *   - CHV_FMT_NV12: 2 planes of 1 and 2 components;
 *   - CHV_FMT_Y420P: 3 planes of 1 component.
 * The two 4:2:0 families are PLANE-WISE: every plane of `src` is resampled to the size of the corresponding plane of `dst` as an image of its
 * own, with the (in, out) tables of its own width and height, every component through the same chain (horizontal then vertical pass, one
 * fused multiply-add per tap, convert_uchar_sat_rte) — no colour conversion, no chroma re-siting, no cross-plane term; all planes in one launch.
 * Errors (nothing is launched, nothing is written): a `dst` of any other format or plane structure, or a target plane that fails a plane
 * check -> CHV_ERR_BAD_TARGET; a `src` whose format and plane structure are not `dst`'s (NV12 -> BGRA, BGRA -> NV12, NV12 -> y420p ...), or a
 * source plane that fails a plane check -> CHV_ERR_BAD_INPUT; a build without the planar kernels -> CHV_ERR_NOT_IMPLEMENTED for the 4:2:0
 * families.  Reductions whose 8 x 4 output tile needs more than 160 KB of staged 4-byte source (about 24:1 on one axis, about 17:1 on both at
 * once) are refused with CHV_ERR_INVALID_VALUE — the rule applies to every plane's own sizes, one refused plane refuses the picture. */
int chv_scale_lanczos(chv_context *ctx, const chv_image *dst, const chv_image *src);
/* n resizes of ONE geometry and ONE format (every src of one size, every dst of one size, all of dsts[0]'s family) in one launch per chunk;
 * same bytes as n calls of chv_scale_lanczos.  Other geometries in the list, a 4:2:0 picture in a list of 4-component planes, a 4-component
 * plane or the other 4:2:0 format in a list of 4:2:0 pictures -> CHV_ERR_INVALID_VALUE, nothing is launched.
 * A chunk is what fits one descriptor slot: CHV_LANCZOS_BATCH_CHUNK (dst, src) pairs of 4-component planes, 62 NV12 pictures (2 plane pairs
 * each) or 41 y420p pictures (3 plane pairs each). */
#define CHV_LANCZOS_BATCH_CHUNK 64
int chv_scale_lanczos_batch(chv_context *ctx, const chv_image *dsts, const chv_image *srcs, int n);
/* Lanczos-3 resize of one BGRA or RGBA plane INTO an NV12 or y420p picture of `dst`'s size, in one launch: the encoder side's rendition.
 * the codes chv_scale_lanczos would write for `src` -> plane 0 of `dst`, red, green and blue taken by `src->format`;
 * luma of every pixel and Cb, Cr of the rounded mean of the 2 x 2 codes a chroma texel covers through the integer matrix of section 4.5 for
 * `opts->colorspace & 3` (opts == NULL: BT.601 limited).  Alpha is not used; nothing is blended with what `dst` held.  Stream order, upload
 * dependencies and a pass's held work are those of chv_scale_lanczos.
 * Errors (nothing is launched, nothing is written):
 *   - `dst` is not CHV_FMT_NV12 with 2 planes (1 and 2 components) or CHV_FMT_Y420P with 3 planes (1 component), a target plane fails a plane
 *     check, or a chroma plane is not max(1, w / 2) x max(1, h / 2) of plane 0's w x h                        -> CHV_ERR_BAD_TARGET;
 *   - `src` is not one 4-component plane whose format is CHV_FMT_BGRA or CHV_FMT_RGBA, or that plane fails a plane check -> CHV_ERR_BAD_INPUT;
 *   - a reduction chv_scale_lanczos refuses for `src` -> plane 0 of `dst` (the 160 KB rule above)            -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit                                                                        -> CHV_ERR_NOT_IMPLEMENTED. */
int chv_scale_lanczos_to_yuv(chv_context *ctx, const chv_image *dst, const chv_image *src, const chv_kernel_opts *opts);
/* n such conversions of ONE geometry, ONE source format, ONE target format and the one colourspace of `opts` in one launch per chunk; same bytes
 * as n calls of chv_scale_lanczos_to_yuv.  Another geometry, source format or target format in the list -> CHV_ERR_INVALID_VALUE, nothing is
 * launched; every other error as above; n == 0 is a no-op.  A chunk is what fits one descriptor slot: 83 pictures into NV12 (3 planes each) or
 * 62 into y420p (4 planes each). */
int chv_scale_lanczos_to_yuv_batch(chv_context *ctx, const chv_image *dsts, const chv_image *srcs, int n, const chv_kernel_opts *opts);
/* An encoder LADDER: n_rungs renditions of each of n sources, all of them in one launch per route.  dsts[r * n + i] is
 * rung r of source i; the call writes the bytes of n_rungs x n calls of chv_scale_lanczos_to_yuv(ctx, &dsts[r * n + i], &srcs[i], opts).
 * One list, one shape: all sources have one size and one format (BGRA or RGBA), all targets one format (NV12 or y420p), all targets of a rung
 * one size; rungs may have any sizes (reductions, 1:1, enlargements, the size of another rung).  A violation, n_rungs < 0, n_rungs >
 * CHV_LADDER_MAX_RUNGS, n < 0 or a NULL list with non-zero counts -> CHV_ERR_INVALID_VALUE; n_rungs == 0 or n == 0 is a no-op.  Every other
 * error is chv_scale_lanczos_to_yuv's, picture by picture (CHV_ERR_BAD_TARGET, CHV_ERR_BAD_INPUT, CHV_ERR_INVALID_VALUE for a rung the 160 KB
 * rule refuses, CHV_ERR_NOT_IMPLEMENTED without the kernel unit, after validation).  All or nothing: one refused rung refuses the ladder, nothing
 * is launched and nothing is written to any rung.  Stream order, upload dependencies and a pass's held work as chv_scale_lanczos_to_yuv_batch.
 * Launches: the rungs that take the wave-per-strip route leave in one launch, the rungs that take the tile route in at most one more, per chunk.
 * A chunk is what fits one descriptor slot of CHV_LADDER_SLOT_BYTES, a picture being its n_rungs x planes target planes and its source plane
 * (stored once) of CHV_LADDER_PLANE_BYTES each: CHV_LADDER_CHUNK(n_rungs, planes) pictures, planes = 2 for NV12 and 3 for y420p.  A longer
 * list is split along the PICTURES: all rungs of a picture leave in one chunk. */
#define CHV_LADDER_MAX_RUNGS 8
#define CHV_LADDER_SLOT_BYTES 5984
#define CHV_LADDER_PLANE_BYTES 24
#define CHV_LADDER_CHUNK(n_rungs, planes) (CHV_LADDER_SLOT_BYTES / (((n_rungs) * (planes) + 1) * CHV_LADDER_PLANE_BYTES))
int chv_scale_lanczos_to_yuv_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n, const chv_kernel_opts *opts);
/* The LADDER of the two 4:2:0 families of chv_scale_lanczos: n_rungs renditions of each of n NV12 or y420p sources as
 * pictures of the SAME format, all of them in one launch per route.  dsts[r * n + i] is rung r of source i; the call writes the bytes of
 * n_rungs x n calls of chv_scale_lanczos(ctx, &dsts[r * n + i], &srcs[i]): every plane resampled plane-wise with the tables of its own width and
 * height, no colour arithmetic.  One list, one shape: all sources have one size and one format, all targets that format, all targets of a rung
 * one size; rungs may have any sizes (reductions, 1:1, enlargements, the size of another rung).
 * Errors (all or nothing: every rung of every picture is validated and every rung's route is computed before the first launch; a refused
 * ladder launches nothing and writes nothing):
 *   - dsts[0] is not CHV_FMT_NV12 with 2 planes (1 and 2 components) or CHV_FMT_Y420P with 3 planes (1 component each) — this entry has no
 *     4-component family, a BGRA or RGBA dsts[0] is refused here — or a target plane fails a plane check         -> CHV_ERR_BAD_TARGET;
 *   - targets that differ in format, sources that differ in format or size, a rung whose targets differ in size, n_rungs < 0, n_rungs >
 *     CHV_LADDER_MAX_RUNGS, n < 0, a NULL list with non-zero counts                                               -> CHV_ERR_INVALID_VALUE;
 *   - sources that are consistently not the targets' format or plane structure, a source plane that fails a plane check -> CHV_ERR_BAD_INPUT;
 *   - a rung for which the 160 KB rule of chv_scale_lanczos refuses any plane                                     -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                           -> CHV_ERR_NOT_IMPLEMENTED.
 * n_rungs == 0 or n == 0 is a no-op.  Stream order, upload dependencies and a pass's held work as chv_scale_lanczos_batch.
 * Launches: the rungs that take the wave-per-strip route leave in one launch, the rungs that take the tile route in at most one more, per chunk
 * (a rung's route is the one its single call takes).  A chunk is what fits one descriptor slot, a picture being its n_rungs x planes target
 * planes and its `planes` source planes (stored once): CHV_PLANAR_LADDER_CHUNK(n_rungs, planes) pictures, planes = 2 for NV12 and 3 for
 * y420p.  A longer list is split along the PICTURES: all rungs of a picture leave in one chunk. */
#define CHV_PLANAR_LADDER_CHUNK(n_rungs, planes) (CHV_LADDER_SLOT_BYTES / ((((n_rungs) + 1) * (planes)) * CHV_LADDER_PLANE_BYTES))
int chv_scale_lanczos_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n);
/* Lanczos-3 BETWEEN the two 4:2:0 packings: any of the four (source packing, target packing) pairs of NV12 and
 * y420p.  A 4:2:0 picture of either packing has three LOGICAL 1-component images Y, Cb and Cr — NV12: Cb and Cr are components 0 and 1 of plane
 * 1, y420p: planes 1 and 2; chroma images are max(1, w / 2) x max(1, h / 2) as everywhere else.  Each logical plane of src is resampled to the
 * size of the same logical plane of dst exactly as chv_scale_lanczos resamples a 1-component plane: its own tables per axis from its own width
 * and height, horizontal then vertical pass, fmaf per tap from 0 with taps ascending, indices clamped to the plane's edge, float intermediate,
 * convert_uchar_sat_rte.  No colour arithmetic, no re-siting, no cross-plane term: the bytes are those chv_scale_lanczos writes for the
 * same-format pair of the same sizes, stored in the other packing; at equal sizes the call is an exact repack.  Same-format pairs (NV12 -> NV12,
 * y420p -> y420p) are accepted and forwarded: they write the bytes of chv_scale_lanczos / chv_scale_lanczos_ladder.
 * chv_scale_lanczos_420_ladder: dsts[r * n + i] is rung r of source i; the call writes the bytes of n_rungs x n single calls.  All sources have
 * one size and one format, all targets one format (which may differ from the sources'), all targets of a rung one size; rungs may have any
 * sizes.  All or nothing; n_rungs == 0 or n == 0 is a no-op.
 * Errors (nothing launched, nothing written):
 *   - dst is not CHV_FMT_NV12 with 2 planes (1 and 2 components) or CHV_FMT_Y420P with 3 planes (1 component each), a target plane fails a plane
 *     check, a y420p target whose planes 1 and 2 differ in width or height                                        -> CHV_ERR_BAD_TARGET;
 *   - the same conditions on src                                                                                  -> CHV_ERR_BAD_INPUT;
 *   - targets of a ladder that differ in format, sources that differ in format or size, a rung whose targets differ in size, n_rungs < 0,
 *     n_rungs > CHV_LADDER_MAX_RUNGS, n < 0, a NULL list with non-zero counts, a rung for which the 160 KB rule of chv_scale_lanczos refuses
 *     any logical plane                                                                                           -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                           -> CHV_ERR_NOT_IMPLEMENTED.
 * Stream order, upload dependencies, a pass's held work and table lifetime as chv_scale_lanczos_batch.  The entries read no switch: a rung
 * takes the wave-per-strip route when no logical plane has more than 22 taps on an axis and the tile route otherwise.
 * Launches of a cross pair: one per route per chunk, at most two per chunk.  A chunk is what fits one descriptor slot, a picture being its
 * n_rungs x target planes + source planes records: CHV_420_LADDER_CHUNK(n_rungs, dst_planes, src_planes) pictures, planes = 2 for NV12 and 3
 * for y420p (for same-format lists it equals CHV_PLANAR_LADDER_CHUNK).  A longer list is split along the PICTURES. */
#define CHV_420_LADDER_CHUNK(n_rungs, dst_planes, src_planes) (CHV_LADDER_SLOT_BYTES / (((n_rungs) * (dst_planes) + (src_planes)) * CHV_LADDER_PLANE_BYTES))
int chv_scale_lanczos_420(chv_context *ctx, const chv_image *dst, const chv_image *src);
int chv_scale_lanczos_420_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n);
/* Lanczos-3 from EVERYTHING the decoder makes into the two 4:2:0 packings: `dst` is an NV12 or y420p picture exactly as
 * chv_scale_lanczos_420 checks it, `src` a picture of one of
 *   - CHV_FMT_NV21:                  2 planes (1 and 2 components); Y is plane 0, Cb byte 1 and Cr byte 0 of each texel of plane 1;
 *   - CHV_FMT_Y422P, CHV_FMT_Y444P:  3 planes of 1 component: Y, Cb, Cr.  The plane sizes the caller gives are taken as they are (a decoder
 *                                    gives w / 2 x h for 4:2:2 and w x h for 4:4:4); Cb and Cr must agree;
 *   - CHV_FMT_YUVS (bytes Y0 Cb Y1 Cr) and CHV_FMT_ZVUY (bytes Cb Y0 Cr Y1): 1 plane described with width = the picture's width in pixels,
 *                                    components = 2 (bytes per pixel), pitch >= 2 x width.  The width must be even; Y is the bytes 0, 2, 4, ...
 *                                    (yuvs) or 1, 3, 5, ... (zvuy) of a row, Cb the bytes 1, 5, 9, ... or 0, 4, 8, ..., Cr the bytes 3, 7, 11, ... or
 *                                    2, 6, 10, ...; the chroma images are width / 2 x height.  These are FFmpeg's byte orders for YUYV422 and
 *                                    UYVY422, because a decoder is where such frames come from; the component lists of
 *                                    sample.pict.linux.swift:283-286 disagree with them;
 *   - CHV_FMT_NV12, CHV_FMT_Y420P:   accepted and forwarded to chv_scale_lanczos_420 / chv_scale_lanczos_420_ladder: their bytes, their launchers,
 *                                    their counters.
 * Every source has three LOGICAL 1-component images Y, Cb and Cr.  Each is resampled to the size of the same logical image of dst exactly as
 * chv_scale_lanczos resamples a 1-component plane: its own tables per axis from its own width and height, horizontal then vertical pass, fmaf
 * per tap from 0 with taps ascending, indices clamped to the image's edge, float intermediate, convert_uchar_sat_rte.  No colour arithmetic, no
 * re-siting, no cross-plane term.  At equal picture sizes therefore: Y is an exact copy (or unpack); NV21 -> NV12 is an exact byte swap of the
 * chroma plane and NV21 -> y420p an exact de-interleave; a 4:2:2 source's chroma is untouched horizontally and reduced 2:1 vertically; a 4:4:4
 * source's chroma is reduced 2:1 on both axes — a 12-tap Lanczos, not a box.
 * chv_scale_lanczos_to_420_ladder: dsts[r * n + i] is rung r of source i; the call writes the bytes of n_rungs x n single calls.  All sources have
 * one size and one format, all targets one format, all targets of a rung one size.  All or nothing; n_rungs == 0 or n == 0 is a no-op.
 * Errors (nothing launched, nothing written):
 *   - as chv_scale_lanczos_420 for dst                                                                            -> CHV_ERR_BAD_TARGET;
 *   - a source that is none of the seven formats with the plane and component counts above (BGRA and RGBA are chv_scale_lanczos_to_yuv's), a
 *     source plane that fails a plane check, Cb and Cr of different size, a packed source of odd width           -> CHV_ERR_BAD_INPUT;
 *   - differing formats or sizes within a list, a bad count, a NULL list with non-zero counts, n_rungs > CHV_LADDER_MAX_RUNGS, a rung for which
 *     the 160 KB rule of chv_scale_lanczos refuses ANY logical image (a 4:4:4 source's chroma is reduced twice as hard as its luma, so it can
 *     be refused where luma passes)                                                                               -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation (forwarded sources still work)                            -> CHV_ERR_NOT_IMPLEMENTED.
 * Stream order, upload dependencies, a pass's held work and table lifetime as chv_scale_lanczos_batch.  The entries read no switch: a rung
 * takes the wave-per-strip route when no logical image has more than 22 taps on an axis and no staged row exceeds 64 vectors at its source's
 * tap stride of 1, 2 or 4 bytes, and the tile route otherwise.  Launches: one per route per chunk, at most two per chunk, counted by
 * "lanczos_to_420_launches" (chv_debug_get_counter; process-wide; forwarded sources do not touch it).  A chunk is
 * CHV_420_LADDER_CHUNK(n_rungs, dst_planes, src_planes) pictures with src_planes of 1, 2 or 3.  A longer list is split along the PICTURES. */
int chv_scale_lanczos_to_420(chv_context *ctx, const chv_image *dst, const chv_image *src);
int chv_scale_lanczos_to_420_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n);
/* Lanczos-3 from the two 10-bit 4:2:0 formats into the two 8-bit 4:2:0 packings ("hbd": high bit depth): `dst` is an
 * NV12 or y420p picture exactly as chv_scale_lanczos_420 checks it, `src` a picture of one of
 *   - CHV_FMT_P010:     2 planes.  Plane 0 is w x h texels of components = 2 (one little-endian 16-bit word: Y), plane 1 is
 *                       max(1, w / 2) x max(1, h / 2) texels of components = 4 (two words: Cb, then Cr).  The code of a sample is word >> 6; the
 *                       low six bits are ignored whatever they hold;
 *   - CHV_FMT_Y420P10:  3 planes of components = 2 (FFmpeg's yuv420p10le): Y, Cb, Cr.  Cb and Cr must agree in size.  The code of a sample is
 *                       word & 1023; the high six bits are ignored.
 * The start address (buffer + offset) and the pitch of every source plane must be even.  8-bit sources are not forwarded: this entry has only
 * its own two formats.
 * Every source has three LOGICAL images Y, Cb and Cr of 10-bit codes 0..1023.  Each is resampled to the size of the same logical image of dst
 * exactly as chv_scale_lanczos resamples a 1-component plane: its own tables per axis from its own width and height, horizontal then vertical
 * pass, fmaf per tap from 0 with taps ascending, indices clamped to the image's edge, float intermediate; the code enters the chain as an
 * exact float.  The value v that leaves the vertical chain is stored as convert_uchar_sat_rte(v * 0.25f): the product is exact, so this rounds
 * once, ties to even, and saturates at 255.  No dither, no colour arithmetic, no re-siting, no cross-plane term.  At equal picture sizes
 * therefore every stored byte is min(rint(code / 4), 255) of the sample at its place: codes 1022 and 1023 give 255, codes 2, 6, 10, ... are ties
 * and go to the even neighbour.
 * chv_scale_lanczos_hbd_to_420_ladder: dsts[r * n + i] is rung r of source i; the call writes the bytes of n_rungs x n single calls.  All sources
 * have one size and one format, all targets one format, all targets of a rung one size.  All or nothing; n_rungs == 0 or n == 0 is a no-op.
 * Errors (nothing launched, nothing written):
 *   - as chv_scale_lanczos_420 for dst                                                                            -> CHV_ERR_BAD_TARGET;
 *   - a source that is neither of the two formats with the plane and component counts above, a source plane that fails a plane check, an odd
 *     start address or pitch, Cb and Cr of different size                                                         -> CHV_ERR_BAD_INPUT;
 *   - differing formats or sizes within a list, a bad count, a NULL list with non-zero counts, n_rungs > CHV_LADDER_MAX_RUNGS, a rung for which
 *     the 160 KB rule of chv_scale_lanczos (applied to sizes, unchanged) refuses any logical image                -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                           -> CHV_ERR_NOT_IMPLEMENTED.
 * Stream order, upload dependencies, a pass's held work and table lifetime as chv_scale_lanczos_batch.  The entries read no switch: the route
 * comes from geometry alone, by the rule of chv_scale_lanczos_to_420 with tap strides of 2 bytes (luma, y420p10 chroma) and 4 bytes (P010
 * chroma).  Launches: one per route per chunk, at most two per chunk, counted by "lanczos_hbd_launches" (chv_debug_get_counter; process-wide).
 * A chunk is CHV_420_LADDER_CHUNK(n_rungs, dst_planes, src_planes) pictures.  A longer list is split along the PICTURES. */
int chv_scale_lanczos_hbd_to_420(chv_context *ctx, const chv_image *dst, const chv_image *src);
int chv_scale_lanczos_hbd_to_420_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n);
/* Lanczos-3 resize of one NV12 or y420p picture INTO a BGRA or RGBA plane of `dst`'s size, in one launch: the decoder side's rendition
 * (DESIGN.md section 4.4.6).  The logical planes Y, Cb and Cr of `src` (NV12: Cb and Cr are components 0 and 1 of plane 1; y420p: planes 1
 * and 2) are each resampled to dst's w x h exactly as chv_scale_lanczos resamples a 1-component plane — the chroma planes straight from
 * max(1, w / 2) x max(1, h / 2) of the source's w x h, every plane with its own tables per axis from its own width and height, horizontal then
 * vertical pass, fmaf per tap from 0 with taps ascending, indices clamped to the plane's edge, float intermediate, convert_uchar_sat_rte; no
 * re-siting, no cross-plane term.  The three CODES of a pixel go through the integer matrix of section 4.2 for `opts->colorspace & 3`
 * (opts == NULL: BT.601 limited); the pixel is stored as B, G, R, 255 (CHV_FMT_BGRA) or R, G, B, 255 (CHV_FMT_RGBA).  Nothing is blended with
 * what `dst` held.  Stream order, upload dependencies, a pass's held work and table lifetime are those of chv_scale_lanczos_batch.
 * Errors (nothing is launched, nothing is written):
 *   - `dst` is not one 4-component plane whose format is CHV_FMT_BGRA or CHV_FMT_RGBA, or that plane fails a plane check -> CHV_ERR_BAD_TARGET;
 *   - `src` is not CHV_FMT_NV12 with 2 planes (1 and 2 components) or CHV_FMT_Y420P with 3 planes (1 component each, planes 1 and 2 of one
 *     size), a chroma plane is not max(1, w / 2) x max(1, h / 2) of plane 0's w x h, or a source plane fails a plane check -> CHV_ERR_BAD_INPUT;
 *   - a logical plane whose own (in, out) sizes the 160 KB rule of chv_scale_lanczos refuses                  -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                       -> CHV_ERR_NOT_IMPLEMENTED.
 * The entries read no switch: a picture takes the wave-per-strip route when no logical plane has more than 22 taps on an axis and the tile
 * route otherwise.  chv_scale_lanczos and every other entry keep their statuses: NV12 -> BGRA there stays CHV_ERR_BAD_INPUT. */
int chv_scale_lanczos_from_yuv(chv_context *ctx, const chv_image *dst, const chv_image *src, const chv_kernel_opts *opts);
/* n such conversions of ONE geometry, ONE source format, ONE target format and the one colourspace of `opts` in one launch per chunk; same bytes
 * as n calls of chv_scale_lanczos_from_yuv.  Another geometry, source format or target format in the list -> CHV_ERR_INVALID_VALUE, all or
 * nothing; every other error as above; n == 0 is a no-op.  A chunk is what fits one descriptor slot, counted as chv_scale_lanczos_to_yuv_batch
 * counts it: 83 pictures from NV12 (3 plane records each) or 62 from y420p (4 plane records each). */
int chv_scale_lanczos_from_yuv_batch(chv_context *ctx, const chv_image *dsts, const chv_image *srcs, int n, const chv_kernel_opts *opts);
/* The decoder side's LADDER: n_rungs BGRA or RGBA renditions of each of n NV12 or y420p sources, all of them in one
 * launch per route.  dsts[r * n + i] is rung r of source i; the call writes the bytes of n_rungs x n calls of
 * chv_scale_lanczos_from_yuv(ctx, &dsts[r * n + i], &srcs[i], opts).  All sources have one size and one format, all targets one format, all
 * targets of one rung one size; rungs may have any sizes (reductions, 1:1, enlargements, the size of another rung).  One colourspace per call
 * (opts == NULL: BT.601 limited).  Stream order, upload dependencies, a pass's held work and table lifetime are those of
 * chv_scale_lanczos_from_yuv_batch.  Every rung of every picture is validated, and every rung's route and launch numbers are computed, before
 * the first launch: a refused ladder launches nothing and writes nothing to any rung.
 *   - n_rungs == 0 or n == 0                                                                                   -> no-op, CHV_OK;
 *   - n_rungs < 0, n_rungs > CHV_LADDER_MAX_RUNGS, n < 0, a NULL list with non-zero counts                      -> CHV_ERR_INVALID_VALUE;
 *   - targets that differ in format, sources that differ in format or size, a rung whose targets differ in size -> CHV_ERR_INVALID_VALUE;
 *   - anything else wrong with one picture -> the status chv_scale_lanczos_from_yuv gives it (CHV_ERR_BAD_TARGET, CHV_ERR_BAD_INPUT);
 *   - a rung with a logical plane that the 160 KB rule of chv_scale_lanczos refuses                             -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                        -> CHV_ERR_NOT_IMPLEMENTED.
 * A rung takes the route its single call takes; per chunk the strip rungs leave in one launch and the tile rungs in at most one more
 * ("lanczos_from_yuv_ladder_launches" counts them).  A chunk is what fits one descriptor slot of CHV_LADDER_SLOT_BYTES, a picture being its
 * n_rungs target planes and its src_planes source planes (stored once) of CHV_LADDER_PLANE_BYTES each:
 * CHV_FROM_YUV_LADDER_CHUNK(n_rungs, src_planes) pictures, src_planes = 2 for NV12 and 3 for y420p (with one rung: the batch's 83 and 62).  A
 * longer list is split along the PICTURES: all rungs of a picture leave in one chunk. */
#define CHV_FROM_YUV_LADDER_CHUNK(n_rungs, src_planes) \
    (CHV_LADDER_SLOT_BYTES / (((n_rungs) + (src_planes)) * CHV_LADDER_PLANE_BYTES))
int chv_scale_lanczos_from_yuv_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n,
                                      const chv_kernel_opts *opts);
/* The LADDER of 4-component planes: n_rungs renditions of each of n BGRA or RGBA planes — the canvases
 * tick_bgra_stream writes, for one — all of them in one launch per route.  dsts[r * n + i] is rung r of source i; the call writes the bytes of
 * n_rungs x n calls of chv_scale_lanczos(ctx, &dsts[r * n + i], &srcs[i]) on one 4-component plane each.  All sources have one size, all
 * targets of one rung one size; rungs may have any sizes (reductions, 1:1, enlargements, the size of another rung).  The `format` field of a
 * 4-component image is not read, as in chv_scale_lanczos: bytes keep their component order.  Stream order, upload dependencies, a pass's
 * held work and table lifetime are those of chv_scale_lanczos_batch.  Every rung of every picture is validated, and every rung's route and
 * launch numbers are computed, before the first launch: a refused ladder launches nothing and writes nothing to any rung.
 *   - n_rungs == 0 or n == 0                                                                                   -> no-op, CHV_OK;
 *   - n_rungs < 0, n_rungs > CHV_LADDER_MAX_RUNGS, n < 0, a NULL list with non-zero counts                      -> CHV_ERR_INVALID_VALUE;
 *   - a target that is not exactly one plane of 4 components (a 4:2:0 picture included: this entry has only the 4-component family), or
 *     whose plane fails a check of chv_scale_lanczos                                                           -> CHV_ERR_BAD_TARGET;
 *   - the same conditions on a source                                                                          -> CHV_ERR_BAD_INPUT;
 *   - sources that differ in size, a rung whose targets differ in size                                         -> CHV_ERR_INVALID_VALUE;
 *   - a rung that chv_scale_lanczos refuses for the same sizes (its 160 KB rule, more than 256 taps)            -> CHV_ERR_INVALID_VALUE;
 *   - a build without the kernel unit, after validation                                                        -> CHV_ERR_NOT_IMPLEMENTED.
 * The route is a function of a rung's geometry alone, and not the single call's: a rung takes the wave-per-strip route when neither axis has
 * more than 22 taps, the source is at least 4 texels wide and the staged row of a strip fits 64 vectors — also where its axes have different
 * tap counts, which a single call sends to its tile kernel — and the tile route otherwise.  Per chunk the strip rungs leave in one launch and
 * the tile rungs in at most one more ("lanczos_rgb_ladder_launches" counts them).  A chunk is what fits one descriptor slot of
 * CHV_LADDER_SLOT_BYTES, a picture being its n_rungs target planes and its one source plane (stored once) of CHV_LADDER_PLANE_BYTES each:
 * CHV_RGB_LADDER_CHUNK(n_rungs) pictures (124 with one rung, 27 with eight).  A longer list is split along the PICTURES: all rungs of a
 * picture leave in one chunk. */
#define CHV_RGB_LADDER_CHUNK(n_rungs) (CHV_LADDER_SLOT_BYTES / (((n_rungs) + 1) * CHV_LADDER_PLANE_BYTES))
int chv_scale_lanczos_rgb_ladder(chv_context *ctx, const chv_image *dsts, int n_rungs, const chv_image *srcs, int n);

/* ---- timing (what the "gpu.upload"/"mix.video.compose" StatsReport timers
 *      measure on the host, compute.swift:185-187, mix.video.swift:110-126,
 *      measured on the stream) ------------------------------------------- */
typedef struct chv_event chv_event;
int chv_event_create(chv_context *ctx, chv_event **out);
int chv_event_record(chv_context *ctx, chv_event *ev);
/* Make all later work of `ctx`'s stream wait for `ev` (recorded on any context of the device). */
int chv_event_wait(chv_context *ctx, chv_event *ev);
int chv_event_synchronize(chv_event *ev);
int chv_event_elapsed_ms(chv_event *start, chv_event *stop, float *ms);
int chv_event_destroy(chv_event *ev);
/* Block until every stream of the context's device is idle. */
int chv_device_synchronize(chv_context *ctx);

#ifdef __cplusplus
}
#endif
#endif /* CHIPVIDEO_H */
