/*
 * iqo_hip.h -- C ABI of the MI355X (gfx950) resize backend for libiqo's hot path.
 *
 * This is the drop-in boundary.  It replaces the per-arch implementation SPI of the reference
 * (the `I*ResizerImpl` interface + `*ResizerImpl_new<Arch>()` factories) with plain C entry
 * points: no C++ or torch types, only pointers, sizes, an opaque plan and an int status.
 *
 *   reference (read-only, /root/reference)                  replaced by
 *   -------------------------------------------------------  ---------------------------------
 *   LanczosResizerImpl_new<Arch>() + init()                  iqo_hip_plan_lanczos()
 *       src/IQOLanczosResizerImpl.hpp:10-29,65-75;
 *       src/IQOLanczosResizerImpl_Generic.cpp:291-339
 *   AreaResizerImpl_new<Arch>() + init()                     iqo_hip_plan_area()
 *       src/IQOAreaResizerImpl.hpp:10-27; src/IQOAreaResizerImpl_Generic.cpp:174-220
 *   LinearResizerImpl_new<Arch>() + init()                   iqo_hip_plan_linear()
 *       src/IQOLinearResizerImpl.hpp:10-27; src/IQOLinearResizerImpl_Generic.cpp:157-191
 *   I*ResizerImpl::resize(srcSt, src, dstSt, dst)            iqo_hip_resize()  (host pointers)
 *       src/IQOLanczosResizerImpl_Generic.cpp:369-454 etc.   iqo_hip_resize_device() (batched,
 *                                                            device pointers, async on a stream)
 *   delete m_Impl  (src/IQOLanczosResizer.cpp:39-42)         iqo_hip_plan_destroy()
 *   HWCap CPUID dispatch (src/IQOHWCap.cpp:32-53)            iqo_hip_available()
 *
 * Semantics: output bytes are identical to the reference's Generic implementation
 * (IQO*ResizerImpl_Generic) for the same inputs.  All functions return IQO_HIP_OK (0) or a
 * negative status; the library never falls back to a CPU path.
 *
 * Threading: a plan may be used from one host thread at a time (like the reference impl, whose
 * work row makes it non-re-entrant, IQOLanczosResizerImpl_Generic.cpp:279); distinct plans are
 * independent.  Device-pointer calls are asynchronous on `stream` (a hipStream_t, or NULL for
 * the default stream).
 */
#ifndef IQO_HIP_H
#define IQO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQO_HIP_OK 0
#define IQO_HIP_EINVAL (-1)     /* bad argument (zero size, bad degree, null pointer, ...) */
#define IQO_HIP_ENODEV (-2)     /* no gfx950 device / HIP runtime unusable */
#define IQO_HIP_ENOMEM (-3)     /* host or device allocation failed */
#define IQO_HIP_EHIP (-4)       /* a HIP runtime call or kernel launch failed */
#define IQO_HIP_EUNSUP (-5)     /* shape or layout not supported (e.g. > 65535 frames) */

enum { IQO_METHOD_LANCZOS = 0, IQO_METHOD_AREA = 1, IQO_METHOD_LINEAR = 2 };

/* Kernel families a plan can dispatch to (iqo_hip_plan_desc.kernel). */
enum {
    IQO_KERNEL_GENERAL = 0,     /* any shape, any layout: one workgroup per output row (fallback) */
    IQO_KERNEL_LANCZOS_STREAM = 1, /* integer ratio, 1 phase: row-band walker, register window */
    IQO_KERNEL_AREA_INT = 2,    /* integer ratio area */
    IQO_KERNEL_LINEAR_UP2 = 3,  /* exact 2x bilinear upsampling */
    IQO_KERNEL_TILE = 4,        /* general ratios, any layout: separable tiles (TH rows x CT columns) */
    IQO_KERNEL_WALK = 5,        /* general ratios, 4-byte aligned sources: wave walker, per-wave LDS ring */
    IQO_KERNEL_LANCZOS_UP2 = 6, /* exact 2x Lanczos-2/3 upscale: register-window streamer, every row and column in-kernel */
    IQO_KERNEL_LANCZOS_D32 = 7, /* exact 3:2 Lanczos-3 downscale: register-window streamer, borders in-kernel */
    IQO_KERNEL_AREA_D32 = 8,    /* exact 3:2 Area downscale: one wave per strip, no window */
    IQO_KERNEL_LANCZOS_U23 = 9, /* exact 2:3 Lanczos-3 upscale: register-window streamer, borders in-kernel */
    IQO_KERNEL_LINEAR_U23 = 10, /* exact 2:3 Linear upscale: clamped halo, no border code */
    IQO_KERNEL_LANCZOS_D31 = 11, /* exact 3:1 Lanczos-2/3 downscale: register window, symmetric taps, borders in-kernel */
    IQO_KERNEL_RYX = 12,         /* exact vertical ratio (9:4), tabled columns: register window + LDS work row */
    IQO_KERNEL_RYG = 13,         /* downscales by 1..2 (e.g. 1080 -> 768 rows), tabled rows and columns: shifting
                                    register window + LDS work row */
    IQO_KERNEL_PACKED_TILE = 14, /* packed pixels (2..4 channels), any layout: separable tiles, work rows de-interleaved
                                    per channel, 4 pixels x all channels per thread */
    IQO_KERNEL_PACKED_GENERAL = 15 /* packed pixels, any shape, any layout: IQO_KERNEL_GENERAL per channel (fallback) */
};

typedef struct iqo_hip_plan iqo_hip_plan;

typedef struct {
    int method;
    int device;
    size_t srcW, srcH, dstW, dstH;
    int tapsX, tapsY;       /* reference coefficient counts (m_NumCoefsX/Y) */
    int phasesX, phasesY;   /* reference table counts (m_NumTablesX/Y) */
    int kernel;             /* IQO_KERNEL_* used for full frames with aligned layouts */
    int bandsPerFrame;      /* fast-path row bands per frame (tuning) */
    int tileRows;           /* output rows per tile of IQO_KERNEL_TILE (option "tile_rows"; 0 = no tile tables) */
} iqo_hip_plan_desc;

/* Number of usable gfx950 devices (0 when none or the runtime is unusable). */
int iqo_hip_available(void);

/* Plan = coefficient tables + index maps built on the host; the tables a kernel reads from device
 * memory are uploaded to `device` once, on the first launch that needs them.  Destroyed plans are
 * kept in a small process-wide cache (options reset to their defaults) and returned again for an
 * identical request, so constructing a resizer per call, as the reference benchmark does, does not
 * rebuild tables.
 *
 * Shapes without a pinned answer.  Linear upscales above 2x read outside the reference's rows:
 * plans are built, the output is unpinned.  Lanczos shapes whose top border band exceeds the
 * output, ceil((tapsY / 2 - 1) * dstH / srcH) > dstH (the vertical window is taller than the source,
 * e.g. degree 8, 115x18 -> 16x6), make the reference write rows past dstH: every plan constructor
 * below (lanczos, packed, yuv420, nv12) and every iqo_host_* query returns IQO_HIP_EINVAL for them.
 * The same bound on the X axis only classifies columns and is accepted. */
int iqo_hip_plan_lanczos(unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                         size_t pxScale, int device, iqo_hip_plan **out);
int iqo_hip_plan_area(size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device, iqo_hip_plan **out);
int iqo_hip_plan_linear(size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device, iqo_hip_plan **out);
/* Interleaved U8 pixels, `channels` bytes per pixel (1..4; RGB, RGBA, the UV plane of NV12).  Every
 * channel is resized independently; channel c of the output is byte-identical to the planar resize
 * of channel c.  channels == 1 is exactly iqo_hip_plan_lanczos/area/linear.  Widths are in PIXELS,
 * strides in BYTES (srcSt >= srcW*channels, dstSt >= dstW*channels), in every call that takes the
 * plan: iqo_hip_resize_device, iqo_hip_resize, iqo_hip_resize_band, iqo_hip_band_src_rows,
 * iqo_hip_plan_prepare / _query / _set_option / _destroy.  degree / pxScale: Lanczos only.
 * IQO_HIP_EINVAL for channels outside 1..4.  Plans with channels > 1 run IQO_KERNEL_PACKED_TILE,
 * or IQO_KERNEL_PACKED_GENERAL where the tile tables do not take the shape or "force_general" is
 * set; no base or stride alignment is required. */
int iqo_hip_plan_packed(int method, unsigned degree, int channels, size_t srcW, size_t srcH,
                        size_t dstW, size_t dstH, size_t pxScale, int device, iqo_hip_plan **out);
int iqo_hip_plan_channels(const iqo_hip_plan *plan);   /* 1 for every other constructor */
void iqo_hip_plan_destroy(iqo_hip_plan *plan);

int iqo_hip_plan_query(const iqo_hip_plan *plan, iqo_hip_plan_desc *desc);

/* Upload the plan's device tables now (one allocation + one blocking copy on the plan's device)
 * instead of inside the first resize call that needs them.  Call it before capturing resize calls
 * into a hipGraph or issuing them on a stream that must not synchronise with the host: the lazy
 * upload would otherwise do a hipMalloc and a blocking null-stream copy inside that first call
 * (and report IQO_HIP_ENOMEM there).  Plans whose kernels take their coefficients as kernel
 * arguments (the specialised fast kernels) have nothing to upload; the call is then a no-op. */
int iqo_hip_plan_prepare(iqo_hip_plan *plan);

/* Options: "force_general" (0/1: every shape through IQO_KERNEL_GENERAL), "bands" (row bands per
 * frame, 0 = auto) and "host_stage" (host-pointer path of frames >= 4 MiB: 0 the HIP runtime's own
 * pageable copies (default), 1 the pinned-staging band pipeline).  Every option changes speed
 * only, never the output bytes.  IQO_HIP_EINVAL for an unknown key or value.
 * With IQO_HIP_TUNING=1 in the environment the call also takes the A/B keys of
 * libiqo_amd/csrc/abi.hip (kernel family switches "tile", "walk", "up2", "d32", "a32", "u23",
 * "l23", "d31", "ryx", "ryg", "ryu"; schedules "tile_rows", "stack", "rounds", "tail", "prefetch",
 * "ratio_prefetch", "ryx_split", "ryx_adj", "ryx_cpt", "ryx_uc", "ryg_cpt", "ryu_run",
 * "stream_variant", "lanes", "chunk_frames"), which the tests and tuning scripts use; they are not
 * part of the supported interface. */
int iqo_hip_plan_set_option(iqo_hip_plan *plan, const char *key, long value);

/* Drop-in resize with HOST pointers (byte strides), synchronous: H2D, kernels, D2H. */
int iqo_hip_resize(iqo_hip_plan *plan, size_t srcSt, const uint8_t *src, size_t dstSt, uint8_t *dst);

/* ---- Layout limits.  Frame strides are unlimited (64-bit) for every kernel.  Within a frame most kernel
 * families address rows with 32-bit byte offsets, so each family limits the row strides and the SPAN of a
 * call: the bytes from the first byte of the source window (destination band) to the last byte touched,
 * (rows - 1) * stride + srcW * channels (dstW * channels), the rows being the source window's or the
 * band's.  The largest accepted values, 0 = unlimited:
 *
 *   family (IQO_KERNEL_*)                          srcSpan, dstSpan         srcSt        dstSt
 *   GENERAL, AREA_INT, PACKED_GENERAL              0                        0            0
 *   TILE, PACKED_TILE                              2^31 - 1                 2^24 - 1     2^31 - 1
 *   LANCZOS_STREAM, LINEAR_UP2                     IQO_HIP_DROP_OFFSET - 1  DROP - 1     DROP - 1
 *   WALK (source row rounded up to 4 bytes)        IQO_HIP_DROP_OFFSET - 1  2^24 - 1     DROP - 1
 *   LANCZOS_UP2 / _D32 / _D31 / _U23, LINEAR_U23,
 *   AREA_D32, RYX, RYG                             IQO_HIP_DROP_OFFSET - 1  2^24 - 1     2^24 - 1
 *
 * IQO_HIP_DROP_OFFSET is the byte offset these kernels give an access that must not happen; a span that
 * reached it would turn such an access into a real one.  Which family a call runs depends on the plan,
 * its options and the alignment of the layout (iqo_hip_plan_query, iqo_host_kernel_for_layout).
 * iqo_host_layout_limits reports the row of a family (host-only; IQO_HIP_EINVAL for an unknown family or a
 * null pointer); the launch functions test against the same table (libiqo_amd/csrc/kernels.hpp). */
#define IQO_HIP_DROP_OFFSET 0x7ff00000
typedef struct iqo_hip_layout_limits {
    uint64_t srcSpanMax, dstSpanMax;   /* bytes, first to last of the window / band; 0 = unlimited */
    uint64_t srcStMax, dstStMax;       /* row strides, bytes; 0 = unlimited */
} iqo_hip_layout_limits;
int iqo_host_layout_limits(int kernel, iqo_hip_layout_limits *out);

/* Batched resize of nFrames frames resident in device memory, asynchronous on `stream`.
 * Frame f reads dSrc + f*srcFrameSt and writes dDst + f*dstFrameSt.
 * IQO_HIP_EINVAL: a null pointer, srcSt < srcW*channels, dstSt < dstW*channels, or a layout beyond the
 * limits above of the family the call runs (source window: the rows iqo_hip_band_src_rows names for the
 * whole frame).  On IQO_HIP_EINVAL nothing is launched and the destination is untouched. */
int iqo_hip_resize_device(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt,
                          const uint8_t *dSrc, size_t dstSt, size_t dstFrameSt, uint8_t *dDst,
                          void *stream);

/* Packed plans (channels 2..4) straight to a model's input: the batched resize above, stored as
 * normalised PLANAR float tensors [frame][plane][row][column] instead of interleaved bytes.  With
 * u8(f, y, x, c) the byte iqo_hip_resize_device writes for the same plan and source,
 *
 *   out(f, p, y, x) = cvt( fl32( fl32( (float)u8(f, y, x, order[p]) * scale[p] ) + bias[p] ) )
 *
 * two separately rounded fp32 operations (not a fused multiply-add); cvt is the identity for
 * IQO_OUT_F32 and round-to-nearest-even to fp16 / bf16 otherwise (overflow gives +-inf).  This is
 * numpy's u8.astype(float32) * float32(s) + float32(b), then .astype(float16) (or torch's
 * .to(bfloat16)), bit for bit.  (v/255 - mean)/std is scale = 1/(255 std), bias = -mean/std; order
 * reorders channels (BGR -> RGB: {2, 1, 0}), repeats them or drops some (planes < channels).
 *
 * Element (f, p, y, x) is at dDst + f*dstFrameSt + p*dstPlaneSt + y*dstRowSt + x*elem, elem = 4 or 2
 * bytes, every stride in BYTES.  dDst and the strides need no alignment beyond the element size
 * (the kernels store 16 / 8 bytes per thread where the addresses allow and single elements
 * otherwise).  Asynchronous on `stream`; the plan's tables are uploaded as for iqo_hip_resize_device
 * (iqo_hip_plan_prepare beforehand for graph capture).  The option "force_general" applies.
 *
 * Plans with channels 2..4 only: a planar (1-channel) plan returns IQO_HIP_EUNSUP -- planar plans
 * dispatch to sixteen kernel families, none of which has the float epilogue; planar sources go through
 * iqo_hip_resize_planes_norm_device below.
 * IQO_HIP_EINVAL: a null plan, dSrc, dDst or norm; an unknown dtype; planes outside 1..4; an order[p]
 * outside 0..channels-1; a non-finite scale[p] or bias[p] (p < planes; entries from `planes` on are
 * ignored); dDst or a destination stride that is no multiple of elem; srcSt < srcW*channels;
 * dstRowSt < dstW*elem; dstPlaneSt < dstH*dstRowSt; dstFrameSt < planes*dstPlaneSt when nFrames > 1;
 * a source frame, or a float frame (from its first element to the end of its last plane's last row),
 * that reaches 2^31 bytes; srcSt >= 2^24.  On any error nothing is launched and the destination is
 * untouched. */
enum { IQO_OUT_F32 = 1, IQO_OUT_F16 = 2, IQO_OUT_BF16 = 3 };
typedef struct {
    int dtype;                 /* IQO_OUT_* */
    int planes;                /* 1..4 output planes */
    int order[4];              /* order[p] in 0..channels-1: the source channel of plane p (repeats allowed) */
    float scale[4], bias[4];   /* per output plane, finite */
} iqo_hip_norm;
int iqo_hip_resize_device_norm(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt,
                               const uint8_t *dSrc, const iqo_hip_norm *norm, size_t dstRowSt,
                               size_t dstPlaneSt, size_t dstFrameSt, void *dDst, void *stream);

/* ---- Planar U8 frames straight to the same normalised planar float tensors: [F, P, H, W] bytes as an
 * image decoder leaves them (P = 3 planar RGB, P = 1 grey), or the Y plane of a video frame.
 *
 * `plan` is a 1-channel plan: from iqo_hip_plan_lanczos / _area / _linear, from iqo_hip_plan_packed with
 * channels == 1, or plane 0 of an NV12 / I420 plan (iqo_hip_nv12_plane(p, 0), iqo_hip_yuv_plane(p, 0):
 * both are ordinary 1-channel plans built by the constructors above, so luma-only input to a model
 * needs no chroma work).  Source plane c (0 <= c < srcPlanes, srcPlanes in 1..4) of frame f starts at
 * dSrc + f*srcFrameSt + c*srcPlaneSt with rows srcSt bytes apart.  Sources are only read, so planes may
 * alias or lie apart (a crop view, the Y plane inside an NV12 frame); srcPlaneSt is ignored when
 * srcPlanes == 1.  With u8(f, c, y, x) exactly the byte iqo_hip_resize_device writes for the same plan
 * with source plane (f, c) as its frame,
 *
 *   out(f, p, y, x) = cvt( fl32( fl32( (float)u8(f, norm->order[p], y, x) * scale[p] ) + bias[p] ) )
 *
 * which is iqo_hip_resize_device_norm's contract word for word (two separately rounded fp32 operations,
 * nearest-even to fp16 / bf16, overflow to +-inf, the same destination addressing and alignment), with
 * order[p] the SOURCE PLANE of output plane p: repeats (grey -> three planes), drops (RGBA planes -> RGB)
 * and permutations (BGR -> RGB) are allowed.
 *
 * Two passes on `stream`, no allocation and no synchronisation in either (capturable after
 * iqo_hip_plan_prepare): the plan's own resize of every source plane that `order` references, through
 * the path of iqo_hip_resize_device (so whatever kernel family the layout gets), into `workspace`, then
 * one memory-bound kernel from the workspace to dDst.  A plane that `order` does not reference is not
 * resized.  When every plane is referenced and srcFrameSt == srcPlanes*srcPlaneSt (the contiguous
 * tensor) the first pass is one batch of nFrames*srcPlanes frames; otherwise one batch per referenced
 * plane.  `workspace` is device memory of at least
 * iqo_hip_planes_norm_workspace_bytes(dstW, dstH, srcPlanes, nFrames) bytes, any alignment, contents
 * unspecified afterwards; it may be reused by later calls on the same stream.  The query is host-only,
 * saturates at SIZE_MAX instead of wrapping and returns SIZE_MAX for srcPlanes outside 1..4 (or
 * dstW / dstH >= 2^31).
 *
 * IQO_HIP_EUNSUP: a plan whose channels are not 1 (packed plans have iqo_hip_resize_device_norm).
 * IQO_HIP_EINVAL: a null plan, dSrc, dDst, norm or workspace; srcPlanes outside 1..4; everything
 * iqo_hip_resize_device_norm rejects of a norm and its destination, with order[p] outside
 * 0..srcPlanes-1; srcSt < srcW; srcSt >= 2^24; a source plane that reaches 2^31 bytes; workspaceBytes
 * below the query's value.  nFrames == 0 returns IQO_HIP_OK after the checks.  Every check runs before
 * the first launch: on any error nothing is launched and the destination is untouched. */
size_t iqo_hip_planes_norm_workspace_bytes(size_t dstW, size_t dstH, int srcPlanes, size_t nFrames);
int iqo_hip_resize_planes_norm_device(iqo_hip_plan *plan, size_t nFrames, int srcPlanes, size_t srcSt,
                                      size_t srcPlaneSt, size_t srcFrameSt, const uint8_t *dSrc,
                                      const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt,
                                      size_t dstFrameSt, void *dDst, void *workspace, size_t workspaceBytes,
                                      void *stream);

/* Source rows [*srcRow0, *srcRow0 + *srcRows) that output rows [dstRow0, dstRow0 + dstRows)
 * read (the halo of a row band).  Host-only, no device work. */
int iqo_hip_band_src_rows(const iqo_hip_plan *plan, size_t dstRow0, size_t dstRows, size_t *srcRow0,
                          size_t *srcRows);

/* Row-band resize (multi-GPU sharding by output rows): computes global output rows
 * [dstRow0, dstRow0 + dstRows) of each frame.  dSrcWindow points at global source row srcRow0
 * (as returned by iqo_hip_band_src_rows, or any window containing it); dDstBand points at the
 * band's first row.  Rows are computed with their GLOBAL indices, so a banded result is
 * byte-identical to the unsharded one.  IQO_HIP_EINVAL if the window starts below the band's
 * first source row; the kernels read no row past the end of the band's window.
 * The layout limits above apply to the band: the source span runs from row srcRow0 to the last row the
 * band reads, the destination span over the band's dstRows rows, so a frame whose whole span is over a
 * limit can still be resized band by band.  IQO_HIP_EINVAL for a band beyond them; on IQO_HIP_EINVAL
 * nothing is launched and the destination is untouched. */
int iqo_hip_resize_band(iqo_hip_plan *plan, size_t nFrames, size_t dstRow0, size_t dstRows,
                        size_t srcRow0, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrcWindow,
                        size_t dstSt, size_t dstFrameSt, uint8_t *dDstBand, void *stream);

/* ---- YUV 4:2:0 (I420) three-plane resize: the reference benchmark's workload
 * (benchmark/benchmark.cpp:131-229, sample/resize_yuv420p.cpp:121-163): Y srcW x srcH -> dstW x dstH,
 * U and V srcW/2 x srcH/2 -> dstW/2 x dstH/2 with the same method; Lanczos chroma uses pxScale 2.
 * The reference composes three resizer objects; here one plan holds the luma and chroma plans. */
typedef struct iqo_hip_yuv_plan iqo_hip_yuv_plan;
int iqo_hip_plan_yuv420(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                        int device, iqo_hip_yuv_plan **out);
void iqo_hip_yuv_plan_destroy(iqo_hip_yuv_plan *plan);
/* Plane 0 = the luma plan, 1 = the chroma plan (for iqo_hip_plan_set_option / _query), 2 = the
 * full-grid chroma plan of IQO_CHROMA_FULL (NULL before iqo_hip_yuv_plan_set_chroma built it). */
iqo_hip_plan *iqo_hip_yuv_plane(iqo_hip_yuv_plan *plan, int plane);
/* Device-resident batch, asynchronous on `stream`: frame f's planes start at srcY/srcU/srcV +
 * f*srcFrameSt (likewise dst).  All three planes go in ONE launch when the plane kernels have a
 * fused instantiation (*fused = 1; the fast kernels of every BASELINE shape do), else one launch
 * per plane (*fused = 0).  `fused` may be NULL.
 * IQO_HIP_EINVAL: a null pointer, a stride below its row, or a plane whose layout is beyond the layout
 * limits (above iqo_hip_resize_device) of the family that plane runs; the fused launch counts every row
 * of a source plane as its window.  All three planes are checked before the first launch: on
 * IQO_HIP_EINVAL nothing is launched and no destination plane is touched. */
int iqo_hip_resize_yuv420_device(iqo_hip_yuv_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                 size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                 size_t dstStY, size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstU,
                                 uint8_t *dstV, void *stream, int *fused);
/* Host pointers, synchronous: the three planes through the pipelined host path of iqo_hip_resize. */
int iqo_hip_resize_yuv420(iqo_hip_yuv_plan *plan, size_t srcStY, const uint8_t *srcY, size_t srcStUV,
                          const uint8_t *srcU, const uint8_t *srcV, size_t dstStY, uint8_t *dstY, size_t dstStUV,
                          uint8_t *dstU, uint8_t *dstV);

/* ---- NV12: a planar Y plane (srcW x srcH) and ONE interleaved UV plane (srcW/2 x srcH/2 pixels of
 * 2 bytes), as the video decode blocks write it.  Y runs the planar plan with all its kernels at
 * pxScale 1; UV runs a 2-channel packed plan at half size (Lanczos: pxScale 2, as the I420 chroma
 * planes above), so U and V are byte-identical to the I420 planes' results.  Two launches on
 * `stream`.  Strides in bytes (srcStUV >= 2 * (srcW/2)). */
typedef struct iqo_hip_nv12_plan iqo_hip_nv12_plan;
int iqo_hip_plan_nv12(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                      int device, iqo_hip_nv12_plan **out);
void iqo_hip_nv12_plan_destroy(iqo_hip_nv12_plan *plan);
/* Plane 0 = the luma plan, 1 = the packed UV plan (for iqo_hip_plan_set_option / _query), 2 = the
 * full-grid UV plan of IQO_CHROMA_FULL (NULL before iqo_hip_nv12_plan_set_chroma built it). */
iqo_hip_plan *iqo_hip_nv12_plane(iqo_hip_nv12_plan *plan, int plane);
/* Device-resident batch, asynchronous on `stream`: frame f's planes start at srcY / srcUV +
 * f*srcFrameSt (likewise dst).
 * IQO_HIP_EINVAL: a null pointer, a stride below its row, or a plane whose layout is beyond the layout
 * limits (above iqo_hip_resize_device) of the family that plane runs.  Both planes are checked before the
 * first launch: on IQO_HIP_EINVAL nothing is launched and neither destination plane is touched. */
int iqo_hip_resize_nv12_device(iqo_hip_nv12_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                               size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcUV, size_t dstStY,
                               size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstUV, void *stream);

/* ---- NV12 / I420 straight to RGB: the resize above, then ONE integer YUV -> RGB definition, stored as
 * packed RGB(A) bytes or as the normalised planar float tensors of iqo_hip_resize_device_norm -- what a
 * model takes from a video decoder, without a float pass in between.
 *
 * Let Y(f, y, x), U(f, j, i), V(f, j, i) be exactly the bytes iqo_hip_resize_nv12_device /
 * iqo_hip_resize_yuv420_device write for the same plan and source: Y at dstW x dstH, chroma at
 * cw x ch = dstW/2 x dstH/2.  Chroma is replicated to the output grid (nearest): pixel (y, x) takes
 * sample (min(y >> 1, ch - 1), min(x >> 1, cw - 1)); the min matters for odd dstW / dstH only.  With
 * y' = Y - yOff, u = U - 128, v = V - 128 in int32 and >> an arithmetic (floor) shift,
 *
 *   R = clamp255((cY y' + cRV v         + 8192) >> 14)
 *   G = clamp255((cY y' - cGU u - cGV v + 8192) >> 14)
 *   B = clamp255((cY y' + cBU u         + 8192) >> 14)
 *
 *   standard               yOff     cY    cRV    cGU    cGV    cBU
 *   IQO_CS_BT601_LIMITED     16  19077  26149   6419  13320  33050
 *   IQO_CS_BT601_FULL         0  16384  22970   5638  11700  29032
 *   IQO_CS_BT709_LIMITED     16  19077  29372   3494   8731  34610
 *   IQO_CS_BT709_FULL         0  16384  25802   3069   7670  30402
 *
 * round(k 2^14) of the standards' real coefficients (libiqo_amd/csrc/colorspace.hpp holds the table for
 * host and device code).  The full-range standards map grey (u = v = 0) to itself; the limited-range
 * ones map 16 to 0 and 235 to 255.
 *
 * The calls take the source arguments of the resize entries, then where the result goes:
 *   _rgb_   packed bytes, `channels` (3 or 4) per pixel, dstSt >= dstW*channels; byte c of a pixel is
 *           order[c] of {0 R, 1 G, 2 B, 3 the constant 255} (RGB {0,1,2}, BGRA {2,1,0,3}, ...); entries
 *           of order from `channels` on are ignored.
 *   _norm_  iqo_hip_resize_device_norm's contract (iqo_hip_norm, strides, the two separately rounded
 *           fp32 operations, the fp16 / bf16 rounding) on the R, G, B bytes as a 3-channel source:
 *           order[p] in 0..2.
 * Neither form needs the destination aligned beyond its element size.
 *
 * Two passes on `stream`: the planes are resized into `workspace` (device memory of at least
 * iqo_hip_yuv_rgb_workspace_bytes(dstW, dstH, nFrames) bytes, any alignment, contents unspecified
 * afterwards), then one kernel writes the destination.  No call allocates or synchronises: after
 * iqo_hip_plan_prepare on both sub-plans they can be captured into a hipGraph.  The option
 * "force_general" of the sub-plans applies to the first pass.  The I420 calls report in *fused (may be
 * NULL) whether the first pass was one launch, as iqo_hip_resize_yuv420_device.
 *
 * IQO_HIP_EINVAL: a null plan, source, destination, workspace, order or norm; an unknown standard;
 * channels outside 3..4; an order[c] outside 0..3 (c < channels); what iqo_hip_resize_device_norm rejects
 * of a norm and its destination (dtype, planes, order[p] outside 0..2, non-finite scale or bias,
 * alignment to the element size, strides below their contents, a destination frame that reaches 2^31
 * bytes); dstSt < dstW*channels, dstFrameSt < dstH*dstSt when nFrames > 1; a source stride below its
 * row, a source plane that reaches 2^31 bytes or a source stride >= 2^24; workspaceBytes below the
 * query's value.  On any error nothing is launched and the destination is untouched. */
enum { IQO_CS_BT601_LIMITED = 0, IQO_CS_BT601_FULL = 1, IQO_CS_BT709_LIMITED = 2, IQO_CS_BT709_FULL = 3 };
/* How the four calls bring chroma to the output grid; a property of the NV12 / I420 plan.
 *
 * IQO_CHROMA_REPLICATE (the default): the definition above.
 * IQO_CHROMA_FULL: chroma is filtered straight to the output grid (4:4:4) instead of being resized to
 * half size and doubled.  Y is exactly the bytes of the plan's Y plane, as above.  U and V are exactly
 * the bytes a resizer of the plan's method and degree writes for srcW/2 x srcH/2 -> dstW x dstH (the
 * 2-channel packed resizer for NV12, the planar one for I420, which agree); Lanczos uses pxScale 1 --
 * pxScale 2 keeps a half-size chroma output in step with luma, but here the output grid is the luma
 * grid, and pxScale 2 would cut Lanczos-3 to one lobe on down-scales.  Pixel (y, x) takes chroma sample
 * (y, x): no shift and no clamp of the index.  The matrix, the rounding and the clamps are unchanged.
 * The resizers map centre to centre, so chroma is treated as sited at the centre of its 2 x 2 luma
 * block, as the plane resizes treat it; left-sited chroma is not addressed.
 *
 * iqo_hip_*_plan_set_chroma selects the mode for iqo_hip_resize_{nv12,yuv420}_{rgb,norm}_device only;
 * the plane resizes (iqo_hip_resize_nv12_device, iqo_hip_resize_yuv420_device, iqo_hip_resize_yuv420)
 * are the same in either mode.  The first IQO_CHROMA_FULL builds one more sub-plan, srcW/2 x srcH/2 ->
 * dstW x dstH at pxScale 1 (NV12: 2-channel packed; I420: planar, run for U and then for V), which
 * iqo_hip_nv12_plane / iqo_hip_yuv_plane return as plane 2 (NULL before that) for
 * iqo_hip_plan_prepare, _query and _set_option; it is kept when the mode goes back.  Call it before the
 * plan is used from other threads or captured into a graph.  In IQO_CHROMA_FULL the first pass is one
 * launch per plane (NV12 two, I420 three; *fused reports 0), and the workspace is larger:
 * iqo_hip_yuv_rgb_workspace_bytes_chroma with the plan's mode is what workspaceBytes is checked against.
 *
 * Returns (the mode keeps its value on any error): IQO_HIP_EINVAL for a null plan or a mode other than
 * the two; IQO_HIP_EUNSUP for Linear with dstW > 2*(srcW/2) or dstH > 2*(srcH/2), a Linear up-scale of
 * chroma above 2x, which has no pinned answer; and what the plan constructor returns for the chroma
 * shape -- IQO_HIP_EINVAL for a Lanczos shape it rejects, which exist under NV12 / I420 plans it accepts
 * (Lanczos-3 16x3 -> 16x3: the full-grid chroma plane is 8x1 -> 16x3). */
enum { IQO_CHROMA_REPLICATE = 0, IQO_CHROMA_FULL = 1 };
int iqo_hip_nv12_plan_set_chroma(iqo_hip_nv12_plan *plan, int mode);
int iqo_hip_yuv_plan_set_chroma(iqo_hip_yuv_plan *plan, int mode);
/* The plan's mode; IQO_HIP_EINVAL for a null plan. */
int iqo_hip_nv12_plan_chroma(const iqo_hip_nv12_plan *plan);
int iqo_hip_yuv_plan_chroma(const iqo_hip_yuv_plan *plan);
/* Host-only, no GPU: the IQO_KERNEL_* family of the full-grid chroma sub-plan of such a plan
 * (interleavedUV != 0: NV12's packed plan; 0: I420's planar plan, 16-byte-aligned layout), or the
 * negative status set_chroma(IQO_CHROMA_FULL) would return. */
int iqo_host_yuv_chroma_full_kernel(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                                    int interleavedUV);
/* Host-only.  The layout of the workspace is internal. */
size_t iqo_hip_yuv_rgb_workspace_bytes(size_t dstW, size_t dstH, size_t nFrames);
/* ... for a plan in chroma mode `mode`: IQO_CHROMA_REPLICATE is the value above; IQO_CHROMA_FULL holds
 * U and V at dstH rows of dstW samples (rows padded as Y's), three bytes per output pixel.  Saturates
 * at SIZE_MAX instead of wrapping, as the function above; SIZE_MAX for an unknown mode. */
size_t iqo_hip_yuv_rgb_workspace_bytes_chroma(size_t dstW, size_t dstH, size_t nFrames, int mode);
int iqo_hip_resize_nv12_rgb_device(iqo_hip_nv12_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                   size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcUV, int standard,
                                   int channels, const int *order /* [4] */, size_t dstSt, size_t dstFrameSt,
                                   uint8_t *dst, void *workspace, size_t workspaceBytes, void *stream);
int iqo_hip_resize_nv12_norm_device(iqo_hip_nv12_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                    size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcUV, int standard,
                                    const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt, size_t dstFrameSt,
                                    void *dDst, void *workspace, size_t workspaceBytes, void *stream);
int iqo_hip_resize_yuv420_rgb_device(iqo_hip_yuv_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                     size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                     int standard, int channels, const int *order /* [4] */, size_t dstSt,
                                     size_t dstFrameSt, uint8_t *dst, void *workspace, size_t workspaceBytes,
                                     void *stream, int *fused);
int iqo_hip_resize_yuv420_norm_device(iqo_hip_yuv_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                      size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                      int standard, const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt,
                                      size_t dstFrameSt, void *dDst, void *workspace, size_t workspaceBytes,
                                      void *stream, int *fused);
/* Host-only, no GPU: the formula above on n (Y, U, V) triples in plain C++ from the same table;
 * rgb receives 3 n bytes (R, G, B per triple).  IQO_HIP_EINVAL for an unknown standard or a null pointer. */
int iqo_host_yuv_to_rgb(int standard, size_t n, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint8_t *rgb);

/* ---- Packed RGB(A) straight to NV12 / I420: the opposite direction, what a hardware encoder takes from a
 * renderer, a compositor or a generative model.  The packed resize above (iqo_hip_resize_device on a plan of
 * iqo_hip_plan_packed with 3 or 4 channels), then ONE integer RGB -> YUV definition with 4:2:0 chroma.
 *
 * Let P(f, y, x, c) be exactly the bytes iqo_hip_resize_device writes for the same plan and source, and
 * R, G, B = P(.., order[0]), P(.., order[1]), P(.., order[2]).  The IQO_CS_* standards as above, 14-bit
 * coefficients, everything in int32, >> a shift of a non-negative value:
 *
 *   Y = (cYR R + cYG G + cYB B + (yOff << 14) + 8192) >> 14
 *   U = min(255, (cUB B - cUR R - cUG G + (128 << 14) + 8192) >> 14)       (4:4:4, iqo_host_rgb_to_yuv only)
 *   V = min(255, (cVR R - cVG G - cVB B + (128 << 14) + 8192) >> 14)
 *
 * Chroma sample (j, i) of the cw x ch = dstW/2 x dstH/2 (rounded down) planes takes SR, SG, SB, the sums
 * over the resized pixels of rows 2j, 2j+1 and columns 2i, 2i+1, and is rounded once, on the sum:
 *
 *   U = min(255, (cUB SB - cUR SR - cUG SG + (128 << 16) + 32768) >> 16)
 *   V = min(255, (cVR SR - cVG SG - cVB SB + (128 << 16) + 32768) >> 16)
 *
 *   standard               yOff   cYR    cYG   cYB   cUR   cUG   cUB   cVR   cVG   cVB
 *   IQO_CS_BT601_LIMITED     16  4207   8260  1604  2428  4768  7196  7196  6026  1170
 *   IQO_CS_BT601_FULL         0  4899   9617  1868  2765  5427  8192  8192  6860  1332
 *   IQO_CS_BT709_LIMITED     16  2991  10064  1016  1649  5547  7196  7196  6536   660
 *   IQO_CS_BT709_FULL         0  3483  11718  1183  1877  6315  8192  8192  7441   751
 *
 * round(k 2^14) of the real coefficients: Kr, Kg, Kb for Y; Kr/(2(1-Kb)), Kg/(2(1-Kb)), 1/2 for U; 1/2,
 * Kg/(2(1-Kr)), Kb/(2(1-Kr)) for V; limited range scales luma by 219/255 and chroma by 224/255
 * (libiqo_amd/csrc/colorspace.hpp holds the table for host and device code).  Rounded one by one they keep
 * cUR + cUG = cUB, cVG + cVB = cVR and cYR + cYG + cYB = 14071 (limited) / 16384 (full): grey gives
 * U = V = 128, black and white give Y = 16 and 235 (limited) or 0 and 255 (full).  No accumulator is ever
 * negative, so there is no lower clamp and none of Y; limited range stays inside 16..235 / 16..240, and in
 * the full-range standards U and V reach 256 before the min (pure blue, pure red).  The chroma planes are
 * centre-sited, as everywhere in this library: the layout iqo_hip_plan_nv12 / _yuv420 read.  An odd dstW's
 * last column and an odd dstH's last row contribute to Y only.
 *
 * order[k] (k = 0, 1, 2) is the byte of a source pixel that holds R, G, B: RGB(A) {0,1,2}, BGR(A) {2,1,0};
 * distinct values below the plan's channels.  A fourth channel is resized and ignored.  The planes of frame
 * f start at dstY / dstUV (or dstU, dstV) + f*dstFrameSt with rows dstStY and dstStUV bytes apart; they need
 * no alignment beyond a byte.
 *
 * Two passes on `stream`: the plan's own resize into `workspace` (device memory of at least
 * iqo_hip_rgb_yuv_workspace_bytes(dstW, dstH, channels, nFrames) bytes, any alignment, contents unspecified
 * afterwards, layout internal), then one kernel writes the planes.  No call allocates or synchronises:
 * after iqo_hip_plan_prepare they can be captured into a hipGraph.  The plan's options apply to the first
 * pass.
 *
 * IQO_HIP_EUNSUP: a plan whose channels are not 3 or 4.  IQO_HIP_EINVAL: a null plan, source, destination,
 * workspace or order; an unknown standard; an order[k] outside 0..channels-1 or two equal ones; dstW < 2 or
 * dstH < 2; dstStY < dstW; dstStUV < 2*cw (NV12) or < cw (I420); a destination stride or plane (first byte
 * to last byte of one frame) that reaches 2^31 bytes; destination planes that overlap (each plane's bytes,
 * first to last, taken as one range); with nFrames > 1 a dstFrameSt below the distance from the first byte
 * of a frame's lowest plane to the end of its highest; a source stride below its row or >= 2^24, a source
 * frame that reaches 2^31 bytes; workspaceBytes below the query's value.  On any error nothing is launched
 * and the destination is untouched. */
/* Host-only.  Saturates at SIZE_MAX instead of wrapping; SIZE_MAX for channels outside 3..4. */
size_t iqo_hip_rgb_yuv_workspace_bytes(size_t dstW, size_t dstH, int channels, size_t nFrames);
int iqo_hip_resize_rgb_nv12_device(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt,
                                   const uint8_t *src, int standard, const int *order /* [3] */, size_t dstStY,
                                   size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstUV, void *workspace,
                                   size_t workspaceBytes, void *stream);
int iqo_hip_resize_rgb_yuv420_device(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt,
                                     const uint8_t *src, int standard, const int *order /* [3] */, size_t dstStY,
                                     size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstU, uint8_t *dstV,
                                     void *workspace, size_t workspaceBytes, void *stream);
/* Host-only, no GPU: the 4:4:4 form on n (R, G, B) triples (rgb: 3 n bytes) in plain C++ from the same
 * table; y, u, v receive n bytes each.  IQO_HIP_EINVAL for an unknown standard or a null pointer. */
int iqo_host_rgb_to_yuv(int standard, size_t n, const uint8_t *rgb, uint8_t *y, uint8_t *u, uint8_t *v);
/* Host-only, no GPU: the 4:2:0 form on one tight image rgb[h][w][3]; y receives w*h bytes, u and v
 * (w/2)*(h/2) each, tight.  IQO_HIP_EINVAL also for w < 2 or h < 2. */
int iqo_host_rgb_to_yuv420(int standard, size_t w, size_t h, const uint8_t *rgb, uint8_t *y, uint8_t *u, uint8_t *v);

/* ---- Multi-GPU data movement for row-band / image sharding.  The reference
 * splits a frame's output rows over OpenMP threads (src/IQOLanczosResizerImpl_AVX512.cpp:269-308);
 * across GPUs the same split needs each band's source window (halo rows) on its device and the
 * bands gathered back -- byte copies, no reduction, no RCCL collective.
 *
 * Copies nFrames blocks of bytesPerFrame bytes: block f from src + f*srcFrameSt to
 * dst + f*dstFrameSt.  A device < 0 means host memory.  Device to device on different GPUs:
 * hipMemcpyPeerAsync over xGMI when peer access is available, else staged through pinned host
 * memory.  Ordering: every route is ordered after the work already queued on `stream` (of the
 * destination device, or of the source device for device -> host).  The stream-ordered routes
 * (0, 1, 3) are asynchronous on `stream`; the host-staging route (2) first waits for `stream` and
 * the source device, then copies synchronously and has landed when the call returns.  *path (may be NULL) reports the route: 0 same device,
 * 1 peer DMA, 2 host staging, 3 host <-> device. */
int iqo_hip_copy_frames(void *dst, int dstDevice, size_t dstFrameSt, const void *src, int srcDevice,
                        size_t srcFrameSt, size_t bytesPerFrame, size_t nFrames, void *stream, int *path);

/* Cross-process access to another process's device buffer (one process per GPU): an exported
 * handle (64-byte hipIpcMemHandle_t + the pointer's offset in its allocation) is sent through any
 * control channel; the receiver opens it and gets a device pointer for iqo_hip_copy_frames. */
typedef struct {
    unsigned char bytes[64];
    uint64_t offset;
} iqo_hip_ipc_handle;
int iqo_hip_ipc_export(const void *devPtr, iqo_hip_ipc_handle *handle);
int iqo_hip_ipc_open(const iqo_hip_ipc_handle *handle, int device, void **devPtr);
int iqo_hip_ipc_close(void *devPtr, const iqo_hip_ipc_handle *handle);

const char *iqo_hip_strerror(int status);
const char *iqo_hip_version(void);

/* Host-only table query (no GPU needed): the quantised coefficient table the plan would upload
 * for `axis` (0 = X, 1 = Y), widened to int32, phases x taps.  Returns phases*taps or < 0. */
int iqo_host_tables(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                    size_t pxScale, int axis, int *nTaps, int *nPhases, int32_t *buf, size_t cap);

/* Host-only twin of iqo_hip_band_src_rows (no device needed): the source-row halo of output rows
 * [dstRow0, dstRow0 + dstRows) for the given resizer shape. */
int iqo_host_band_src_rows(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                           size_t pxScale, size_t dstRow0, size_t dstRows, size_t *srcRow0, size_t *srcRows);

/* Host-only: which kernel family a full-frame, 16-byte-aligned device call would use. */
int iqo_host_kernel_for(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                        size_t pxScale);

/* as iqo_host_kernel_for, for a source / destination whose base, row stride and frame stride
 * are multiples of srcAlign / dstAlign bytes (powers of two, 1..16) and of nothing larger;
 * IQO_HIP_EINVAL for any other alignment value */
int iqo_host_kernel_for_layout(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW,
                               size_t dstH, size_t pxScale, size_t srcAlign, size_t dstAlign);

/* Host-only: the same for a packed plan of `channels` bytes per pixel (IQO_KERNEL_PACKED_TILE or
 * IQO_KERNEL_PACKED_GENERAL; channels == 1: iqo_host_kernel_for).  < 0 for channels outside 1..4. */
int iqo_host_packed_kernel_for(int method, unsigned degree, int channels, size_t srcW, size_t srcH, size_t dstW,
                               size_t dstH, size_t pxScale);

/* The template instantiation a planar (1-channel) call runs, for the families that have more than one:
 * IQO_KERNEL_TILE, _WALK, _LANCZOS_UP2, _LANCZOS_D32, _AREA_D32, _LANCZOS_U23, _LINEAR_U23, _LANCZOS_D31,
 * _RYX and _RYG.  The fields are the kernels' template parameters by name; one a kernel does not have
 * is 0.  For the other families (the integer-ratio streamers, the general and the packed kernels) only
 * `family` is set.
 *   tile_kernel          NP, LZ                            (LZ 1: Lanczos, 0: Area / Linear)
 *   walk_kernel          NP, VY, NV, LZ
 *   lanczos_up2_kernel   NT, F
 *   lanczos_d32_kernel   PD, VARIANT                       (VARIANT 0: Lanczos-3 taps, 1: Lanczos-2 taps)
 *   lanczos_d31_kernel   PD, VARIANT
 *   lanczos_u23_kernel, linear_u23_kernel, area_d32_kernel   PD
 *   ryx_kernel           LZ, P, Q, T, NP, PD, ADJ, CPT, UC
 *   ryg_kernel           LZ, T, NP, PD, CPT, NL            (sub 0)
 *   ryu_kernel           T, NP, PD, CPT, RUN, KM           (sub IQO_INSTANCE_SUB_RYU: IQO_KERNEL_RYG's upscale
 *                                                           rows walked by window position) */
enum { IQO_INSTANCE_SUB_NONE = 0, IQO_INSTANCE_SUB_RYU = 1 };
typedef struct iqo_hip_instance {
    int family;             /* IQO_KERNEL_* */
    int sub;                /* IQO_INSTANCE_SUB_* */
    int LZ, P, Q, T, NP, PD, ADJ, CPT, UC, NL, RUN, KM, VY, NV, NT, F, VARIANT;
} iqo_hip_instance;

/* The instantiation a full-frame call of `plan` runs with the plan's CURRENT options, when the source /
 * destination base and strides are multiples of srcAlign / dstAlign bytes (powers of two, 1..16) and of
 * nothing larger -- exactly the entry of the family's table that the launch function would run (one
 * lookup serves both).  No launch, no device access.  IQO_HIP_EINVAL for a null plan or descriptor or
 * another alignment value, IQO_HIP_EUNSUP for a packed plan, and IQO_HIP_EINVAL where the resize call
 * itself would be rejected: a forced "ratio_prefetch" depth the kernel does not instantiate. */
int iqo_hip_plan_instance(const iqo_hip_plan *plan, size_t srcAlign, size_t dstAlign, iqo_hip_instance *desc);

/* Host-only twin (no GPU needed): the same for a shape and nOptions options, applied in order through
 * iqo_hip_plan_set_option itself -- so an unknown key, an out-of-range value or (without IQO_HIP_TUNING=1)
 * a tuning key is IQO_HIP_EINVAL here too, as is a shape the plan constructors reject. */
typedef struct iqo_hip_option {
    const char *key;
    long value;
} iqo_hip_option;
int iqo_host_instance_for(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                          size_t pxScale, const iqo_hip_option *options, size_t nOptions, size_t srcAlign,
                          size_t dstAlign, iqo_hip_instance *desc);

/* The grid of one launch, by number: how many workgroups a call starts and how a workgroup's flat id
 * becomes the (column, band, frame) it resizes.  Reported by the launch function itself, run in a query
 * mode that stops before the launch, so the figures are the launch's own.
 *
 * A "unit" is what a kernel decodes its place from: a wave (walker, the exact-ratio kernels: 4 per
 * workgroup), a tile (tile, packed tile) or a whole workgroup (ryx / ryg / ryu, the block-shared Lanczos
 * streamer).  The frame-folding families put units of all frames into one id range and permute the
 * workgroup id L of `blocks` ids for XCD locality:
 *   IQO_GRID_MAP_SPREAD    XCD x = L mod 8 takes a contiguous eighth of [0, blocks): with q = blocks / 8,
 *                          r = blocks mod 8, i = L / 8: x < r ? x (q + 1) + i : r (q + 1) + (x - r) q + i
 *   IQO_GRID_MAP_CHUNKS    chunks of `chunk` = C ids (about one frame's) dealt round-robin over the XCDs:
 *                          with full = blocks / (8 C), an id with i < full C maps to
 *                          (8 (i / C) + x) C + i mod C; the ids from 8 full C on map by SPREAD among
 *                          themselves
 *   IQO_GRID_MAP_XCD_TAIL  block-shared streamer, frames a multiple of 8 and >= 16: XCD x resizes frames
 *                          x, x + 8, ... in `bands` bands each and its last frame in `tailBands` shorter
 *                          ones; gridX = 8 ((frames / 8 - 1) bands + tailBands)
 * Unit u then belongs to frame u / unitsPerFrame; unit ids from `units` on (the last workgroup's spare
 * waves) do nothing.  IQO_GRID_MAP_NONE: the frames are gridY (general, per-wave streamers, area_int,
 * linear_up2, the stacked streamer with framesPerBlock frames per workgroup), the unit fields are 0. */
enum { IQO_GRID_MAP_NONE = 0, IQO_GRID_MAP_SPREAD = 1, IQO_GRID_MAP_CHUNKS = 2, IQO_GRID_MAP_XCD_TAIL = 3 };
typedef struct iqo_hip_launch_grid {
    int family;                      /* IQO_KERNEL_* */
    int map;                         /* IQO_GRID_MAP_* */
    unsigned gridX, gridY, gridZ, block;
    unsigned blocks;                 /* ids the map permutes (map none: gridX) */
    unsigned chunk;                  /* C of IQO_GRID_MAP_CHUNKS, else 0 */
    unsigned unitsPerFrame, unitsPerBlock;
    unsigned units;                  /* the kernel's wave / tile / workgroup count argument */
    int bands, wavesPerRow;          /* 0: the family has none (tile families: bands = tile rows) */
    unsigned framesPerBlock;         /* 1, stacked streamer: frames side by side in a workgroup */
    int tailBands;                   /* IQO_GRID_MAP_XCD_TAIL only */
    unsigned frames;                 /* frames of this launch: min(nFrames, 65535 or "chunk_frames") */
} iqo_hip_launch_grid;

/* The first launch of a call of nFrames frames over output rows [dstRow0, dstRow0 + dstRows) of `plan`
 * with its CURRENT options, aligned base and strides.  Band counts chosen automatically ask the plan's
 * device for the kernel's occupancy, as the call does.  No launch.  IQO_HIP_EINVAL: null arguments, no
 * rows or frames, rows outside the plan, or a call the launcher would reject. */
int iqo_hip_plan_launch_grid(const iqo_hip_plan *plan, size_t nFrames, size_t dstRow0, size_t dstRows,
                             iqo_hip_launch_grid *desc);

/* Host-only twin (no GPU needed), as iqo_host_instance_for: a full-frame call of a shape of `channels`
 * (1: planar, 2 .. 4: packed) with nOptions options.  Without a device an automatic band count takes the
 * occupancy as one workgroup per CU of 256 CUs, a lower bound of the real one: where the count it yields
 * is the one set by the rows (every small shape), the device gives the same. */
int iqo_host_launch_grid(int method, unsigned degree, int channels, size_t srcW, size_t srcH, size_t dstW,
                         size_t dstH, size_t pxScale, const iqo_hip_option *options, size_t nOptions,
                         size_t nFrames, iqo_hip_launch_grid *desc);

/* Workgroups of a launch of the second-pass kernels (YUV -> RGB, RGB -> YUV, planes -> floats): 256 items
 * each; a call of more than IQO_HIP_GRID_STRIDE_BLOCKS * 256 items strides over the rest. */
#define IQO_HIP_GRID_STRIDE_BLOCKS 2048u

/* Host-only: every instantiation of a family, in table order (IQO_KERNEL_RYG: ryg_kernel's, then
 * ryu_kernel's).  The count is 0 for a family with a single kernel and for an unknown family;
 * iqo_host_instance_at is IQO_HIP_EINVAL for a null descriptor or an index outside 0 .. count - 1. */
int iqo_host_instance_count(int family);
int iqo_host_instance_at(int family, int index, iqo_hip_instance *desc);

/* Host-only: 1 when a default-option call of this shape runs the block-shared Lanczos 2:1 streamer with
 * the folded vertical pass -- its own quantised Y table has an outer tap that is twice its neighbour
 * (as u16 values: c2 == 2 c1 in the 10-tap window of Lanczos-3, c1 == 2 c0 in the 12-tap window of
 * Lanczos-4), so the two pair sums enter one multiply-add as P + 2 P'.  0 for every other table and
 * every other kernel; < 0 for a shape the plan constructors reject. */
int iqo_host_lanczos_yfold(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                           size_t pxScale);

/* Fused I420 instantiations: the kernel iqo_hip_resize_yuv420_device runs when it resizes the three
 * planes in one launch.  IQO_YUV420_NONE: plane by plane. */
enum {
    IQO_YUV420_NONE = 0,
    IQO_YUV420_LZ_SYMB10 = 1,  /* Lanczos-3 2:1, Y block-shared symmetric streamer (exactly 4 waves per row) */
    IQO_YUV420_LZ_SYM10 = 2,   /* Lanczos-3 2:1, Y per-wave symmetric streamer */
    IQO_YUV420_LZ_SYMB8 = 3,   /* Lanczos-2 2:1, block-shared */
    IQO_YUV420_LZ_SYM8 = 4,    /* Lanczos-2 2:1, per-wave */
    IQO_YUV420_AREA44 = 5,     /* Area 4:1 x 4:1 */
    IQO_YUV420_AREA22 = 6,     /* Area 2:1 x 2:1 */
    IQO_YUV420_AREA2Y = 7,     /* Area 2:1 columns, any integer row ratio */
    IQO_YUV420_AREA4Y = 8,
    IQO_YUV420_AREA8Y = 9,
    IQO_YUV420_AREA33 = 10,    /* Area 3:1 x 3:1 */
    IQO_YUV420_AREA3Y = 11,
    IQO_YUV420_AREA6Y = 12,
    IQO_YUV420_LIN_D2 = 13,    /* Linear 2:1 */
    IQO_YUV420_LIN_UP2 = 14    /* Linear 2x */
};

/* Host-only: the IQO_YUV420_* instantiation an I420 call of this shape runs with default options and a
 * 16-byte-aligned layout (Y at the given size, U and V at half size; Lanczos chroma: pxScale 2, as
 * iqo_hip_plan_yuv420).  < 0 for a request iqo_hip_plan_yuv420 rejects. */
int iqo_host_yuv420_fused(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH);

/* ---- Crop-and-resize a batch of boxes to ONE output size in one launch (RandomResizedCrop, detector
 * boxes for a second stage, thumbnails of regions).
 *
 * A roi plan fixes method, degree, channels (1, 3 or 4 interleaved bytes per pixel) and dstW x dstH; the
 * source sizes come with each call.  Box i of a call names frame `frame` of nFrames frames of
 * frameW x frameH pixels (frame f at dSrc + f*srcFrameSt, rows srcSt bytes apart) and the rectangle
 * [x, x + w) x [y, y + h) in it.  Output i is, bit for bit, what iqo::{Lanczos,Area,Linear}Resizer
 * (w, h -> dstW, dstH), pixel scale 1, gives on the cropped image, per channel: the box is the whole image
 * for border purposes, pixels outside it never contribute, and the kernel never reads a byte outside the
 * rows of the frames it was given.  With flags bit 0 set, column x of that result is stored at column
 * dstW - 1 - x (a horizontal flip of the output; the resize itself is unchanged).
 *
 *   iqo_hip_resize_rois_device       output i: dstW x dstH pixels of `channels` bytes at dDst + i*dstRoiSt,
 *                                    rows dstSt bytes apart
 *   iqo_hip_resize_rois_norm_device  output i: iqo_hip_resize_device_norm's planar float planes (iqo_hip_norm,
 *                                    order[p] < channels, the same two separately rounded fp32 operations,
 *                                    fp32 / fp16 / bf16) of those bytes; element (i, p, y, x) at
 *                                    dDst + i*dstRoiSt + p*dstPlaneSt + y*dstSt + x*elem.  channels == 1
 *                                    works too (grey -> 3 planes: order {0, 0, 0}).
 *
 * Validity follows the plan constructors, box by box.  IQO_HIP_EINVAL: an empty box, a box outside
 * frameW x frameH, a frame index >= nFrames, an unknown flag bit, a Lanczos box whose top border band is
 * taller than the output (what iqo_hip_plan_lanczos rejects, e.g. Lanczos-3 with h = 1, dstH = 24); Linear
 * up-scales above 2x are accepted as everywhere in this library.  IQO_HIP_EUNSUP: a box whose reference
 * table has more than IQO_HIP_ROI_MAX_TAPS taps on either axis (Lanczos-3 reaches 21:1, Area 128:1); a box
 * whose one work row -- channels x (w + the tap windows' overhang) 16-bit values plus 8 bytes per Y tap --
 * exceeds IQO_HIP_ROI_LDS_BYTES (w up to 8000 at 4 channels); more workgroups than one grid addresses
 * (2^31); frameH*srcSt >= 2^31.  *badRoi (may be null) receives the first offending box, or -1 when an
 * argument of the call itself is at fault: null pointers, srcSt < frameW*channels, dstSt too small for a
 * row, dstRoiSt (or dstPlaneSt) too small for an output, and for the norm form everything
 * iqo_hip_resize_device_norm rejects of a norm and its strides.  On any error nothing is launched and the
 * destination is untouched.  nRois == 0 returns IQO_HIP_OK after the checks
 * (dSrc and dDst may then be null).
 *
 * Asynchronous on `stream`, no allocation in steady state.  The per-call tables (one X table per distinct
 * w, one Y table per distinct h, and a record per box) travel in the call: the plan owns two pinned host
 * arenas with a device arena each, grown when a batch needs more, and a call fills one, copies it with
 * hipMemcpyAsync on `stream`, launches and records an event; arenas alternate, and before one is refilled
 * its event is synchronised, so the host blocks only when it is two calls ahead of the device.  The plan
 * keeps a host cache of axis tables by (axis, length), least recently used dropped beyond a byte cap:
 * repeated lengths cost a memcpy.  Because the tables are per call, a CAPTURING stream gets
 * IQO_HIP_EUNSUP.  A roi plan is NOT thread-safe: one call at a time per plan. */
#define IQO_HIP_ROI_MAX_TAPS 128
#define IQO_HIP_ROI_LDS_BYTES 65536
typedef struct { int frame, x, y, w, h, flags; } iqo_hip_roi;   /* flags bit 0: mirror the output columns */
enum { IQO_ROI_FLIP = 1 };
typedef struct iqo_hip_roi_plan iqo_hip_roi_plan;
int iqo_hip_plan_rois(int method, unsigned degree, int channels, size_t dstW, size_t dstH, int device,
                      iqo_hip_roi_plan **out);
void iqo_hip_roi_plan_destroy(iqo_hip_roi_plan *plan);
int iqo_hip_resize_rois_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                               size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt,
                               const uint8_t *dSrc, size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream,
                               int *badRoi);
int iqo_hip_resize_rois_norm_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                    size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt,
                                    const uint8_t *dSrc, const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt,
                                    size_t dstRoiSt, void *dDst, void *stream, int *badRoi);

/* Host-only CPU twins of the two calls above (host pointers, no stream, no device): they assemble the same
 * arena and walk it in plain C++ with the kernel's integer formulas, so the device calls must equal them
 * byte for byte.  Same status codes and *badRoi. */
int iqo_host_resize_rois(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                         const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                         size_t srcFrameSt, const uint8_t *src, size_t dstSt, size_t dstRoiSt, uint8_t *dst,
                         int *badRoi);
int iqo_host_resize_rois_norm(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                              const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                              size_t srcFrameSt, const uint8_t *src, const iqo_hip_norm *norm, size_t dstSt,
                              size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi);
/* Host-only: what the arena of such a call holds (tightly packed frames: srcSt = frameW*channels). */
typedef struct {
    size_t arenaBytes;    /* header + one record per box + every distinct table once */
    int xTables, yTables; /* distinct X tables (box widths) and Y tables (box heights) */
    unsigned workgroups;  /* the launch's grid */
    size_t ldsBytes;      /* its dynamic LDS: the largest workgroup's */
    size_t recordBytes;   /* bytes of one box record */
} iqo_hip_roi_arena_stats;
int iqo_host_roi_arena_stats(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                             const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                             iqo_hip_roi_arena_stats *stats, int *badRoi);
/* Host-only: what the layout of a call decides for ONE box of w x h pixels (the layout of a one-box call, the
 * box being the whole of a tightly packed frame).  Same status codes as the calls above. */
typedef struct {
    int rows;             /* output rows per workgroup */
    unsigned workgroups;  /* ceil(dstH / rows) */
    size_t ldsBytes;      /* dynamic LDS of one workgroup: rows x (channels x pitchDw x 4 + nYp x 8) */
    int nYp;              /* Y taps per output row, padded to even */
    int np;               /* NP: X coefficient pairs per output column */
    int pitchDw;          /* work-row pitch of one channel, dwords */
} iqo_hip_roi_box_layout;
int iqo_host_roi_box_layout(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t w, size_t h,
                            iqo_hip_roi_box_layout *out);

/* ---- Crop-and-resize boxes of NV12 / I420 frames straight to RGB bytes or normalised tensors, in one launch
 * (decoder frames on the device, a detector's boxes, a classifier's input).
 *
 * A roi yuv plan fixes method, degree, layout (IQO_ROI_NV12: a Y plane and an interleaved UV plane;
 * IQO_ROI_I420: Y, U and V planes) and dstW x dstH.  A call brings nFrames frames of frameW x frameH, both
 * even: the planes of frame 0 as device pointers (dV is not read for NV12), their row strides srcStY and
 * srcStUV, and ONE srcFrameSt that is applied to every plane pointer, as the iqo_hip_resize_nv12_*_device
 * entries do; and nRois boxes with x, y, w, h even and w, h >= 2.  Output i is, bit for bit:
 *
 *   Y    = iqo::{Lanczos,Area,Linear}Resizer (w,   h   -> dstW, dstH), pixel scale 1, on the box of the Y plane
 *   U, V = the same resizer                  (w/2, h/2 -> dstW, dstH), pixel scale 1, on the box of U and of V
 *          (rows y/2 .. (y+h)/2, columns x/2 .. (x+w)/2: chroma centred, filtered to the full output grid)
 *   RGB  = the integer matrix of `standard` (IQO_CS_*, above) of the three bytes of a pixel
 *
 * which is what an NV12 / I420 plan (w, h -> dstW, dstH) with IQO_CHROMA_FULL gives on the cropped frame.  The
 * box is the whole image for border purposes, in luma and in chroma; no byte outside the rows of the given
 * planes is read; IQO_ROI_FLIP mirrors the output columns.  Source pointers and strides need no alignment.
 *
 *   iqo_hip_resize_rois_yuv_rgb_device   `channels` 3 or 4 bytes per pixel, byte c = order[c] of {0 R, 1 G, 2 B,
 *                                        3 the constant 255}, rows dstSt and outputs dstRoiSt bytes apart
 *   iqo_hip_resize_rois_yuv_norm_device  the planar floats of iqo_hip_resize_rois_norm_device of the 3-channel
 *                                        pixel (R, G, B): norm->order[p] in 0 .. 2
 *
 * Validity, box by box (*badRoi names the first offending box).  IQO_HIP_EINVAL: an odd x, y, w or h; w < 2 or
 * h < 2; a box outside the frame; a frame index >= nFrames; an unknown flag bit; a Lanczos box whose luma axes
 * (w, h) or chroma axes (w/2, h/2) iqo_hip_plan_lanczos rejects (Lanczos-3 with h = 2 and dstH = 24: chroma
 * 1 -> 24).  IQO_HIP_EUNSUP: Linear with dstW > w or dstH > h (chroma above 2x: the rule of IQO_CHROMA_FULL, so
 * every accepted Linear box has a pinned answer); more than IQO_HIP_ROI_MAX_TAPS taps on any of the four axes; a
 * band row -- the Y, U and V work rows and both sets of Y-tap records, (pitchY + 2 pitchC) x 4 + (nYpY + nYpC) x 8
 * bytes -- over IQO_HIP_ROI_LDS_BYTES; more than 2^31 workgroups; frameH*srcStY >= 2^31 or
 * (frameH/2)*srcStUV >= 2^31; a capturing stream.  *badRoi = -1 and IQO_HIP_EINVAL for an argument of the call
 * itself: odd frameW or frameH, null pointers, srcStY < frameW, srcStUV < frameW (NV12) or frameW/2 (I420), an
 * unknown standard, channels other than 3 or 4, an order entry outside 0 .. 3, and everything
 * iqo_hip_resize_rois_device (the norm form: with 3 source channels) rejects of the destination.  On any error
 * nothing is launched and the destination is untouched; nRois == 0 returns IQO_HIP_OK after the checks.
 *
 * The plan works as a roi plan: two pinned arenas with a device arena each, one hipMemcpyAsync, one launch and
 * one event per call, no allocation in steady state, NOT thread-safe.  Its table cache serves luma and chroma:
 * a chroma axis of length n shares the table of a luma axis of length n. */
enum { IQO_ROI_NV12 = 0, IQO_ROI_I420 = 1 };
typedef struct iqo_hip_roi_yuv_plan iqo_hip_roi_yuv_plan;
int iqo_hip_plan_rois_yuv(int method, unsigned degree, int layout, size_t dstW, size_t dstH, int device,
                          iqo_hip_roi_yuv_plan **out);
void iqo_hip_roi_yuv_plan_destroy(iqo_hip_roi_yuv_plan *plan);
int iqo_hip_resize_rois_yuv_rgb_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                       size_t nFrames, size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV,
                                       size_t srcFrameSt, const uint8_t *dY, const uint8_t *dUorUV,
                                       const uint8_t *dV /* NULL for NV12 */, int standard, int channels,
                                       const int *order, size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream,
                                       int *badRoi);
int iqo_hip_resize_rois_yuv_norm_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                        size_t nFrames, size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV,
                                        size_t srcFrameSt, const uint8_t *dY, const uint8_t *dUorUV,
                                        const uint8_t *dV /* NULL for NV12 */, int standard, const iqo_hip_norm *norm,
                                        size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt, void *dDst, void *stream,
                                        int *badRoi);
/* Host-only CPU twins (host pointers, no stream, no device): the same arena walked in plain C++ with the
 * kernel's integer formulas.  Same status codes and *badRoi. */
int iqo_host_resize_rois_yuv_rgb(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                 size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                 const uint8_t *v, int standard, int channels, const int *order, size_t dstSt,
                                 size_t dstRoiSt, uint8_t *dst, int *badRoi);
int iqo_host_resize_rois_yuv_norm(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                  const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                  size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                  const uint8_t *v, int standard, const iqo_hip_norm *norm, size_t dstSt,
                                  size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi);
/* Host-only: the arena of such a call on tightly packed frames.  xTables / yTables count every distinct table
 * once, whether luma, chroma or both use it. */
int iqo_host_roi_yuv_arena_stats(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                 iqo_hip_roi_arena_stats *stats, int *badRoi);
/* Host-only: the layout of a one-box call, the box being the whole of a tightly packed w x h frame. */
typedef struct {
    int rows;                /* output rows per workgroup */
    unsigned workgroups;     /* ceil(dstH / rows) */
    size_t ldsBytes;         /* rows x ((pitchDw + 2 pitchDwC) x 4 + (nYp + nYpC) x 8) */
    int nYp, np, pitchDw;    /* luma: Y taps per row (even), X coefficient pairs, work-row pitch in dwords */
    int nYpC, npC, pitchDwC; /* chroma: the same of the (w/2, h/2) tables */
} iqo_hip_roi_yuv_box_layout;
int iqo_host_roi_yuv_box_layout(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t w, size_t h,
                                iqo_hip_roi_yuv_box_layout *out);

/* ---- Boxes into destination rectangles (letterbox, pad to square, aspect-true crops), of both box families.
 *
 * Output i of a fit call is a dstW x dstH canvas.  Rectangle rects[i] = (x, y, w, h) = (ox, oy, iw, ih) of it
 * holds, bit for bit, what the stretch call of the same plan gives for box i with (iw, ih) in place of (dstW,
 * dstH): the resizer (w, h -> iw, ih) on the cropped image per channel; for NV12 / I420 Y (w, h -> iw, ih), U and V
 * (w/2, h/2 -> iw, ih) and the integer matrix.  IQO_ROI_FLIP mirrors the columns inside the rectangle.  Every
 * pixel outside the rectangle is the pad colour: pad[c] is the byte of channel c (packed), or pad[0 .. 2] are R, G,
 * B in output space, stored through `order` as a pixel is, the fourth byte of a 4-byte pixel being 255 (YUV;
 * pad[3] is not read).  The norm forms are byte * scale + bias of that canvas, pad included.  rects == NULL: every
 * rectangle is the whole output (the stretch call's result); pad == NULL: zeros.  rects and pad are host memory,
 * read during the call.
 *
 * The calls take the plans of their stretch twins (one plan serves both kinds of call; its table cache is keyed by
 * (axis, source length, output length)) and their arguments, and reject what they reject with (iw, ih) for
 * (dstW, dstH) -- Lanczos rows without a defined result, Linear above 2x (YUV: iw > w or ih > h), more than
 * IQO_HIP_ROI_MAX_TAPS taps, a band row over IQO_HIP_ROI_LDS_BYTES, a capturing stream -- and, with
 * IQO_HIP_EINVAL and the box in *badRoi, a rectangle that does not lie inside the output or has w or h below 1.
 * The destination checks are the stretch calls'.  Every byte of every canvas is written exactly once: a band
 * workgroup writes its rows of the rectangle and the pad columns left and right of them, and pad workgroups of
 * the same launch write the rows above and below the rectangle, at most padRows rows each (see the layout query). */
typedef struct { int x, y, w, h; } iqo_hip_roi_rect;
int iqo_hip_resize_rois_fit_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                   size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt,
                                   const uint8_t *dSrc, size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream,
                                   int *badRoi, const iqo_hip_roi_rect *rects /* host */, const uint8_t pad[4]);
int iqo_hip_resize_rois_fit_norm_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                        size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt,
                                        const uint8_t *dSrc, const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt,
                                        size_t dstRoiSt, void *dDst, void *stream, int *badRoi,
                                        const iqo_hip_roi_rect *rects /* host */, const uint8_t pad[4]);
int iqo_hip_resize_rois_yuv_fit_rgb_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                           size_t nFrames, size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV,
                                           size_t srcFrameSt, const uint8_t *dY, const uint8_t *dUorUV,
                                           const uint8_t *dV /* NULL for NV12 */, int standard, int channels,
                                           const int *order, size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream,
                                           int *badRoi, const iqo_hip_roi_rect *rects /* host */, const uint8_t pad[4]);
int iqo_hip_resize_rois_yuv_fit_norm_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois /* host */,
                                            size_t nFrames, size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV,
                                            size_t srcFrameSt, const uint8_t *dY, const uint8_t *dUorUV,
                                            const uint8_t *dV /* NULL for NV12 */, int standard,
                                            const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt,
                                            void *dDst, void *stream, int *badRoi,
                                            const iqo_hip_roi_rect *rects /* host */, const uint8_t pad[4]);
/* Host-only CPU twins: the fit arena walked in plain C++.  Same status codes and *badRoi. */
int iqo_host_resize_rois_fit(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                             const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                             size_t srcFrameSt, const uint8_t *src, size_t dstSt, size_t dstRoiSt, uint8_t *dst,
                             int *badRoi, const iqo_hip_roi_rect *rects, const uint8_t pad[4]);
int iqo_host_resize_rois_fit_norm(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                                  const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                                  size_t srcFrameSt, const uint8_t *src, const iqo_hip_norm *norm, size_t dstSt,
                                  size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi,
                                  const iqo_hip_roi_rect *rects, const uint8_t pad[4]);
int iqo_host_resize_rois_yuv_fit_rgb(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                     const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                     size_t srcStY, size_t srcStUV, size_t srcFrameSt, const uint8_t *y,
                                     const uint8_t *uOrUV, const uint8_t *v, int standard, int channels,
                                     const int *order, size_t dstSt, size_t dstRoiSt, uint8_t *dst, int *badRoi,
                                     const iqo_hip_roi_rect *rects, const uint8_t pad[4]);
int iqo_host_resize_rois_yuv_fit_norm(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                      const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                      size_t srcStY, size_t srcStUV, size_t srcFrameSt, const uint8_t *y,
                                      const uint8_t *uOrUV, const uint8_t *v, int standard, const iqo_hip_norm *norm,
                                      size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi,
                                      const iqo_hip_roi_rect *rects, const uint8_t pad[4]);
/* The rectangle of a w x h box in a dstW x dstH output, by one pinned integer rule (64-bit; a caller maps
 * detections back to the frame with these numbers).  IQO_FIT_STRETCH: the whole output.  Letterbox: if
 * w*dstH >= h*dstW then iw = dstW and ih = max(1, (h*dstW + w/2) / w), otherwise ih = dstH and
 * iw = max(1, (w*dstH + h/2) / h); centred (ox = (dstW - iw) / 2, oy = (dstH - ih) / 2, floored) or at the top
 * left (ox = oy = 0).  IQO_HIP_EINVAL: an unknown mode, a null `out`, a zero size, w or h above 2^24, dstW or dstH
 * above 2^20. */
enum { IQO_FIT_STRETCH = 0, IQO_FIT_LETTERBOX = 1, IQO_FIT_LETTERBOX_TOPLEFT = 2 };
int iqo_host_fit_rect(int mode, size_t w, size_t h, size_t dstW, size_t dstH, iqo_hip_roi_rect *out);
/* Host-only: the arenas of fit calls on tightly packed frames (recordBytes: the fit formats'; workgroups: bands and
 * pad workgroups), and what the layout decides for ONE box of w x h pixels going to rectangle *rect (NULL: the
 * whole output) of a dstW x dstH canvas: `box` is what the stretch query reports for (w, h) -> (iw, ih). */
int iqo_host_roi_fit_arena_stats(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                 iqo_hip_roi_arena_stats *stats, int *badRoi, const iqo_hip_roi_rect *rects);
int iqo_host_roi_yuv_fit_arena_stats(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                     const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                     iqo_hip_roi_arena_stats *stats, int *badRoi, const iqo_hip_roi_rect *rects);
typedef struct {
    iqo_hip_roi_box_layout box;
    unsigned padAbove, padBelow;  /* pad workgroups above and below the rectangle: ceil(rows there / padRows) */
    int padRows;                  /* canvas rows one pad workgroup writes, at most */
} iqo_hip_roi_fit_box_layout;
typedef struct {
    iqo_hip_roi_yuv_box_layout box;
    unsigned padAbove, padBelow;
    int padRows;
} iqo_hip_roi_yuv_fit_box_layout;
int iqo_host_roi_fit_box_layout(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t w, size_t h,
                                const iqo_hip_roi_rect *rect, iqo_hip_roi_fit_box_layout *out);
int iqo_host_roi_yuv_fit_box_layout(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t w,
                                    size_t h, const iqo_hip_roi_rect *rect, iqo_hip_roi_yuv_fit_box_layout *out);

/* Drop-in classes (iqo::LanczosResizer, AreaResizer, LinearResizer): how many objects this process constructed on the
 * HIP backend, and on the CPU backend (no gfx950 device) plus the resize() calls of HIP objects that fell back to the
 * CPU (a device failure, or a call the HIP path rejected).  IQO_REQUIRE_HIP=1 makes any CPU use abort;
 * IQO_DROPIN_REPORT=1 prints the counts at exit (libiqo_amd/csrc/resizers.cpp). */
void iqo_dropin_backend_counts(int *hip, int *cpu);

#ifdef __cplusplus
}
#endif
#endif
