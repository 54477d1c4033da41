"""libiqo_amd -- MI355X-native (gfx950) hot path of libiqo's Lanczos / Area / Linear U8 resize.

Python host mirror of the reference's public interface (include/libiqo/*Resizer.hpp), bound
through ctypes to the C ABI in include/iqo_hip.h (libiqo_amd/libiqo_hip.so).  The classes keep
the reference's names, constructor arguments and `resize(srcSt, src, dstSt, dst)` entry point;
`resize_device` adds the batched, device-resident form used for throughput (pointers may come
from torch tensors -- torch is plumbing here, never part of the computation).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is usable, every
call raises `IqoError`.
"""
import ctypes
import os

__all__ = ["IqoError", "LanczosResizer", "AreaResizer", "LinearResizer", "Yuv420Resizer", "Nv12Resizer", "available",
           "lib", "host_tables", "host_kernel_for", "host_packed_kernel_for", "host_yuv420_fused", "host_band_src_rows", "host_instance_for", "host_instances", "Instance", "copy_frames", "ipc_export", "ipc_open",
           "ipc_close", "KERNELS", "YUV420_FUSED", "COPY_PATHS", "LIB_PATH", "Norm", "OUT_F32", "OUT_F16", "OUT_BF16",
           "CS_BT601_LIMITED", "CS_BT601_FULL", "CS_BT709_LIMITED", "CS_BT709_FULL", "COLOR_STANDARDS", "RGB_ORDERS",
           "host_yuv_to_rgb", "yuv_rgb_workspace_bytes", "CHROMA_REPLICATE", "CHROMA_FULL", "CHROMA_MODES",
           "host_chroma_full_kernel", "host_rgb_to_yuv", "host_rgb_to_yuv420", "rgb_yuv_workspace_bytes",
           "SOURCE_ORDERS", "RoiResizer", "Roi", "RoiArenaStats", "host_resize_rois", "host_roi_arena_stats",
           "RoiBoxLayout", "host_roi_box_layout", "ROI_MAX_TAPS", "ROI_LDS_BYTES", "YuvRoiResizer", "ROI_LAYOUTS",
           "RoiYuvBoxLayout", "host_resize_rois_yuv", "host_roi_yuv_arena_stats", "host_roi_yuv_box_layout", "LaunchGrid",
           "RoiRect", "FIT_MODES", "fit_rects", "host_roi_fit_box_layout", "host_roi_yuv_fit_box_layout",
           "host_launch_grid", "GRID_MAPS", "GRID_STRIDE_BLOCKS"]

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# LIBIQO_AMD_LIB selects an alternative build of the same library (A/B experiments only)
LIB_PATH = os.environ.get("LIBIQO_AMD_LIB") or os.path.join(PKG_DIR, "libiqo_hip.so")

KERNELS = {0: "general", 1: "lanczos_stream", 2: "area_int", 3: "linear_up2", 4: "tile", 5: "walk", 6: "lanczos_up2", 7: "lanczos_d32", 8: "area_d32", 9: "lanczos_u23", 10: "linear_u23", 11: "lanczos_d31", 12: "ryx", 13: "ryg", 14: "packed_tile", 15: "packed_general"}
# IQO_YUV420_*: the fused I420 instantiations (one launch for the three planes)
YUV420_FUSED = {0: "none", 1: "lz_symb10", 2: "lz_sym10", 3: "lz_symb8", 4: "lz_sym8", 5: "area44", 6: "area22",
                7: "area2y", 8: "area4y", 9: "area8y", 10: "area33", 11: "area3y", 12: "area6y", 13: "lin_d2",
                14: "lin_up2"}
_METHODS = {"lanczos": 0, "area": 1, "linear": 2}

_c_sz = ctypes.c_size_t
_vp = ctypes.c_void_p


class IqoError(RuntimeError):
    pass


class PlanDesc(ctypes.Structure):
    _fields_ = [("method", ctypes.c_int), ("device", ctypes.c_int), ("srcW", _c_sz), ("srcH", _c_sz),
                ("dstW", _c_sz), ("dstH", _c_sz), ("tapsX", ctypes.c_int), ("tapsY", ctypes.c_int),
                ("phasesX", ctypes.c_int), ("phasesY", ctypes.c_int), ("kernel", ctypes.c_int),
                ("bandsPerFrame", ctypes.c_int), ("tileRows", ctypes.c_int)]


INSTANCE_PARAMS = ("LZ", "P", "Q", "T", "NP", "PD", "ADJ", "CPT", "UC", "NL", "RUN", "KM", "VY", "NV", "NT", "F", "VARIANT")


class Instance(ctypes.Structure):
    """iqo_hip_instance: kernel family, sub-kernel tag and the template parameters by name (0: not a parameter
    of that kernel)."""
    _fields_ = [("family", ctypes.c_int), ("sub", ctypes.c_int)] + [(k, ctypes.c_int) for k in INSTANCE_PARAMS]


# IQO_GRID_MAP_*: how a frame-folding kernel turns a flat workgroup id into a logical one
GRID_MAPS = {0: "none", 1: "spread", 2: "chunks", 3: "xcd_tail"}
# IQO_HIP_GRID_STRIDE_BLOCKS: workgroups (of 256 items) of a second-pass launch; more items are strided over
GRID_STRIDE_BLOCKS = 2048


class LaunchGrid(ctypes.Structure):
    """iqo_hip_launch_grid: the grid of one launch and the numbers its block map decodes with."""
    _fields_ = [("family", ctypes.c_int), ("map", ctypes.c_int), ("gridX", ctypes.c_uint), ("gridY", ctypes.c_uint),
                ("gridZ", ctypes.c_uint), ("block", ctypes.c_uint), ("blocks", ctypes.c_uint), ("chunk", ctypes.c_uint),
                ("unitsPerFrame", ctypes.c_uint), ("unitsPerBlock", ctypes.c_uint), ("units", ctypes.c_uint),
                ("bands", ctypes.c_int), ("wavesPerRow", ctypes.c_int), ("framesPerBlock", ctypes.c_uint),
                ("tailBands", ctypes.c_int), ("frames", ctypes.c_uint)]


def _grid_dict(d):
    out = {k: getattr(d, k) for k, _ in LaunchGrid._fields_}
    out["family"] = KERNELS.get(d.family, d.family)
    out["map"] = GRID_MAPS[d.map]
    return out


class _Option(ctypes.Structure):
    _fields_ = [("key", ctypes.c_char_p), ("value", ctypes.c_long)]


def _instance_dict(d):
    """{"kernel": the kernel's name (ryg / ryu within the ryg family), then its non-zero parameters}."""
    name = "ryu" if d.family == 13 and d.sub == 1 else KERNELS.get(d.family, d.family)
    out = {"kernel": name}
    out.update({k: getattr(d, k) for k in INSTANCE_PARAMS if getattr(d, k)})
    return out


class Norm(ctypes.Structure):
    """iqo_hip_norm: element type, output planes, their source channels and affine maps."""
    _fields_ = [("dtype", ctypes.c_int), ("planes", ctypes.c_int), ("order", ctypes.c_int * 4),
                ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4)]


OUT_F32, OUT_F16, OUT_BF16 = 1, 2, 3  # IQO_OUT_*
CS_BT601_LIMITED, CS_BT601_FULL, CS_BT709_LIMITED, CS_BT709_FULL = 0, 1, 2, 3  # IQO_CS_*
COLOR_STANDARDS = {"bt601": CS_BT601_LIMITED, "bt601-full": CS_BT601_FULL, "bt709": CS_BT709_LIMITED,
                   "bt709-full": CS_BT709_FULL}
# packed byte orders of resize_rgb: the source of each byte of a pixel (0 R, 1 G, 2 B, 3 the constant 255)
RGB_ORDERS = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3)}
# source pixel orders of resize_nv12 / resize_i420: the byte of a packed pixel that holds R, G, B
SOURCE_ORDERS = {"rgb": (0, 1, 2), "bgr": (2, 1, 0)}
# IQO_CHROMA_*: chroma resized to half the output and replicated 2 x 2, or filtered to the full output grid
CHROMA_REPLICATE, CHROMA_FULL = 0, 1
CHROMA_MODES = {"replicate": CHROMA_REPLICATE, "full": CHROMA_FULL}


class Roi(ctypes.Structure):
    """iqo_hip_roi: a rectangle of one frame; flags bit 0 mirrors the output columns."""
    _fields_ = [("frame", ctypes.c_int), ("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int),
                ("h", ctypes.c_int), ("flags", ctypes.c_int)]


class RoiArenaStats(ctypes.Structure):
    """iqo_hip_roi_arena_stats"""
    _fields_ = [("arenaBytes", _c_sz), ("xTables", ctypes.c_int), ("yTables", ctypes.c_int),
                ("workgroups", ctypes.c_uint), ("ldsBytes", _c_sz), ("recordBytes", _c_sz)]


class RoiBoxLayout(ctypes.Structure):
    """iqo_hip_roi_box_layout"""
    _fields_ = [("rows", ctypes.c_int), ("workgroups", ctypes.c_uint), ("ldsBytes", _c_sz), ("nYp", ctypes.c_int),
                ("np", ctypes.c_int), ("pitchDw", ctypes.c_int)]


ROI_MAX_TAPS, ROI_LDS_BYTES = 128, 65536  # IQO_HIP_ROI_MAX_TAPS, IQO_HIP_ROI_LDS_BYTES
ROI_LAYOUTS = {"nv12": 0, "i420": 1}  # IQO_ROI_NV12, IQO_ROI_I420


class RoiYuvBoxLayout(ctypes.Structure):
    """iqo_hip_roi_yuv_box_layout"""
    _fields_ = [("rows", ctypes.c_int), ("workgroups", ctypes.c_uint), ("ldsBytes", _c_sz), ("nYp", ctypes.c_int),
                ("np", ctypes.c_int), ("pitchDw", ctypes.c_int), ("nYpC", ctypes.c_int), ("npC", ctypes.c_int),
                ("pitchDwC", ctypes.c_int)]


class RoiRect(ctypes.Structure):
    """iqo_hip_roi_rect: the rectangle of an output a box goes to."""
    _fields_ = [("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int)]


class RoiFitBoxLayout(ctypes.Structure):
    """iqo_hip_roi_fit_box_layout"""
    _fields_ = [("box", RoiBoxLayout), ("padAbove", ctypes.c_uint), ("padBelow", ctypes.c_uint), ("padRows", ctypes.c_int)]


class RoiYuvFitBoxLayout(ctypes.Structure):
    """iqo_hip_roi_yuv_fit_box_layout"""
    _fields_ = [("box", RoiYuvBoxLayout), ("padAbove", ctypes.c_uint), ("padBelow", ctypes.c_uint),
                ("padRows", ctypes.c_int)]


FIT_MODES = {"stretch": 0, "letterbox": 1, "letterbox-topleft": 2}  # IQO_FIT_*


class IpcHandle(ctypes.Structure):
    """iqo_hip_ipc_handle: hipIpcMemHandle_t bytes + the pointer's offset in its allocation."""
    _fields_ = [("bytes", ctypes.c_ubyte * 64), ("offset", ctypes.c_uint64)]


COPY_PATHS = {0: "same device", 1: "peer DMA (xGMI)", 2: "host staging", 3: "host<->device"}

_lib = None


def lib():
    """Load libiqo_hip.so (raises IqoError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IqoError("libiqo_hip.so not built: run `make -C libiqo_amd` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    pp = ctypes.POINTER(_vp)
    L.iqo_hip_available.restype = ctypes.c_int
    L.iqo_hip_plan_lanczos.argtypes = [ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_plan_area.argtypes = [_c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_plan_linear.argtypes = [_c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_plan_packed.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz,
                                      ctypes.c_int, pp]
    L.iqo_hip_plan_channels.argtypes = [_vp]
    L.iqo_hip_plan_destroy.argtypes = [_vp]
    L.iqo_hip_plan_destroy.restype = None
    L.iqo_hip_plan_query.argtypes = [_vp, ctypes.POINTER(PlanDesc)]
    L.iqo_hip_plan_prepare.argtypes = [_vp]
    L.iqo_hip_plan_set_option.argtypes = [_vp, ctypes.c_char_p, ctypes.c_long]
    L.iqo_hip_resize.argtypes = [_vp, _c_sz, _vp, _c_sz, _vp]
    L.iqo_hip_resize_device.argtypes = [_vp, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _c_sz, _vp, _vp]
    L.iqo_hip_resize_device_norm.argtypes = [_vp, _c_sz, _c_sz, _c_sz, _vp, ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz,
                                             _vp, _vp]
    L.iqo_hip_planes_norm_workspace_bytes.argtypes = [_c_sz, _c_sz, ctypes.c_int, _c_sz]
    L.iqo_hip_planes_norm_workspace_bytes.restype = _c_sz
    # plan, nFrames, srcPlanes, srcSt, srcPlaneSt, srcFrameSt, src, norm, the destination's strides and base,
    # workspace, workspaceBytes, stream
    L.iqo_hip_resize_planes_norm_device.argtypes = [_vp, _c_sz, ctypes.c_int, _c_sz, _c_sz, _c_sz, _vp,
                                                    ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp]
    L.iqo_hip_band_src_rows.argtypes = [_vp, _c_sz, _c_sz, ctypes.POINTER(_c_sz), ctypes.POINTER(_c_sz)]
    L.iqo_hip_resize_band.argtypes = [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _c_sz, _vp, _vp]
    L.iqo_hip_strerror.restype = ctypes.c_char_p
    L.iqo_hip_strerror.argtypes = [ctypes.c_int]
    L.iqo_hip_version.restype = ctypes.c_char_p
    L.iqo_host_tables.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int32), _c_sz]
    L.iqo_host_kernel_for.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz]
    L.iqo_host_kernel_for_layout.argtypes = L.iqo_host_kernel_for.argtypes + [_c_sz, _c_sz]
    L.iqo_hip_plan_instance.argtypes = [_vp, _c_sz, _c_sz, ctypes.POINTER(Instance)]
    L.iqo_host_instance_for.argtypes = L.iqo_host_kernel_for.argtypes + [ctypes.POINTER(_Option), _c_sz, _c_sz, _c_sz,
                                                                         ctypes.POINTER(Instance)]
    L.iqo_hip_plan_launch_grid.argtypes = [_vp, _c_sz, _c_sz, _c_sz, ctypes.POINTER(LaunchGrid)]
    L.iqo_host_launch_grid.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz,
                                       ctypes.POINTER(_Option), _c_sz, _c_sz, ctypes.POINTER(LaunchGrid)]
    L.iqo_host_instance_count.argtypes = [ctypes.c_int]
    L.iqo_host_instance_at.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(Instance)]
    L.iqo_host_band_src_rows.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz,
                                         ctypes.POINTER(_c_sz), ctypes.POINTER(_c_sz)]
    L.iqo_hip_plan_yuv420.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_yuv_plan_destroy.argtypes = [_vp]
    L.iqo_hip_yuv_plan_destroy.restype = None
    L.iqo_hip_yuv_plane.argtypes = [_vp, ctypes.c_int]
    L.iqo_hip_yuv_plane.restype = _vp
    L.iqo_hip_resize_yuv420_device.argtypes = [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp, _vp, _c_sz, _c_sz, _c_sz,
                                               _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int)]
    L.iqo_hip_resize_yuv420.argtypes = [_vp, _c_sz, _vp, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, _vp, _vp]
    L.iqo_host_packed_kernel_for.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz]
    L.iqo_host_yuv420_fused.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz]
    L.iqo_hip_plan_nv12.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_nv12_plan_destroy.argtypes = [_vp]
    L.iqo_hip_nv12_plan_destroy.restype = None
    L.iqo_hip_nv12_plane.argtypes = [_vp, ctypes.c_int]
    L.iqo_hip_nv12_plane.restype = _vp
    L.iqo_hip_resize_nv12_device.argtypes = [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _c_sz, _c_sz, _vp, _vp,
                                             _vp]
    src_nv12 = [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp]        # plan, nFrames, srcStY, srcStUV, srcFrameSt, Y, UV
    src_i420 = src_nv12 + [_vp]                                   # ... Y, U, V
    to_rgb = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _c_sz, _c_sz, _vp, _vp, _c_sz, _vp]
    to_norm = [ctypes.c_int, ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp]
    L.iqo_hip_yuv_rgb_workspace_bytes.argtypes = [_c_sz, _c_sz, _c_sz]
    L.iqo_hip_yuv_rgb_workspace_bytes.restype = _c_sz
    L.iqo_hip_resize_nv12_rgb_device.argtypes = src_nv12 + to_rgb
    L.iqo_hip_resize_nv12_norm_device.argtypes = src_nv12 + to_norm
    L.iqo_hip_resize_yuv420_rgb_device.argtypes = src_i420 + to_rgb + [ctypes.POINTER(ctypes.c_int)]
    L.iqo_hip_resize_yuv420_norm_device.argtypes = src_i420 + to_norm + [ctypes.POINTER(ctypes.c_int)]
    L.iqo_host_yuv_to_rgb.argtypes = [ctypes.c_int, _c_sz, _vp, _vp, _vp, _vp]
    L.iqo_hip_yuv_rgb_workspace_bytes_chroma.argtypes = [_c_sz, _c_sz, _c_sz, ctypes.c_int]
    L.iqo_hip_yuv_rgb_workspace_bytes_chroma.restype = _c_sz
    for name in ("iqo_hip_nv12_plan_set_chroma", "iqo_hip_yuv_plan_set_chroma"):
        getattr(L, name).argtypes = [_vp, ctypes.c_int]
    for name in ("iqo_hip_nv12_plan_chroma", "iqo_hip_yuv_plan_chroma"):
        getattr(L, name).argtypes = [_vp]
    L.iqo_host_yuv_chroma_full_kernel.argtypes = [ctypes.c_int, ctypes.c_uint, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.c_int]
    L.iqo_hip_rgb_yuv_workspace_bytes.argtypes = [_c_sz, _c_sz, ctypes.c_int, _c_sz]
    L.iqo_hip_rgb_yuv_workspace_bytes.restype = _c_sz
    # plan, nFrames, srcSt, srcFrameSt, src, standard, order, dstStY, dstStUV, dstFrameSt, then the planes
    to_yuv = [_vp, _c_sz, _c_sz, _c_sz, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _c_sz, _c_sz, _c_sz]
    L.iqo_hip_resize_rgb_nv12_device.argtypes = to_yuv + [_vp, _vp, _vp, _c_sz, _vp]
    L.iqo_hip_resize_rgb_yuv420_device.argtypes = to_yuv + [_vp, _vp, _vp, _vp, _c_sz, _vp]
    L.iqo_host_rgb_to_yuv.argtypes = [ctypes.c_int, _c_sz, _vp, _vp, _vp, _vp]
    L.iqo_host_rgb_to_yuv420.argtypes = [ctypes.c_int, _c_sz, _c_sz, _vp, _vp, _vp, _vp]
    pi = ctypes.POINTER(ctypes.c_int)
    roi_src = [_c_sz, ctypes.POINTER(Roi), _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _vp]
    roi_host = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz]
    L.iqo_hip_plan_rois.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_roi_plan_destroy.argtypes = [_vp]
    L.iqo_hip_roi_plan_destroy.restype = None
    L.iqo_hip_resize_rois_device.argtypes = [_vp] + roi_src + [_c_sz, _c_sz, _vp, _vp, pi]
    L.iqo_hip_resize_rois_norm_device.argtypes = [_vp] + roi_src + [ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz, _vp,
                                                                    _vp, pi]
    L.iqo_host_resize_rois.argtypes = roi_host + roi_src + [_c_sz, _c_sz, _vp, pi]
    L.iqo_host_resize_rois_norm.argtypes = roi_host + roi_src + [ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz, _vp, pi]
    L.iqo_host_roi_arena_stats.argtypes = roi_host + [_c_sz, ctypes.POINTER(Roi), _c_sz, _c_sz, _c_sz,
                                                      ctypes.POINTER(RoiArenaStats), pi]
    L.iqo_host_roi_box_layout.argtypes = roi_host + [_c_sz, _c_sz, ctypes.POINTER(RoiBoxLayout)]
    # nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, Y, U or UV, V; then the output
    ryuv_src = [_c_sz, ctypes.POINTER(Roi), _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp, _vp]
    ryuv_rgb = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _c_sz, _c_sz, _vp]
    ryuv_norm = [ctypes.c_int, ctypes.POINTER(Norm), _c_sz, _c_sz, _c_sz, _vp]
    L.iqo_hip_plan_rois_yuv.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, _c_sz, _c_sz, ctypes.c_int, pp]
    L.iqo_hip_roi_yuv_plan_destroy.argtypes = [_vp]
    L.iqo_hip_roi_yuv_plan_destroy.restype = None
    L.iqo_hip_resize_rois_yuv_rgb_device.argtypes = [_vp] + ryuv_src + ryuv_rgb + [_vp, pi]
    L.iqo_hip_resize_rois_yuv_norm_device.argtypes = [_vp] + ryuv_src + ryuv_norm + [_vp, pi]
    L.iqo_host_resize_rois_yuv_rgb.argtypes = roi_host + ryuv_src + ryuv_rgb + [pi]
    L.iqo_host_resize_rois_yuv_norm.argtypes = roi_host + ryuv_src + ryuv_norm + [pi]
    L.iqo_host_roi_yuv_arena_stats.argtypes = roi_host + [_c_sz, ctypes.POINTER(Roi), _c_sz, _c_sz, _c_sz,
                                                          ctypes.POINTER(RoiArenaStats), pi]
    L.iqo_host_roi_yuv_box_layout.argtypes = roi_host + [_c_sz, _c_sz, ctypes.POINTER(RoiYuvBoxLayout)]
    # the fit entries: their stretch twins' arguments, then the rectangles and the pad colour
    fit = [ctypes.POINTER(RoiRect), ctypes.POINTER(ctypes.c_ubyte)]
    for name in ("hip_resize_rois_device", "hip_resize_rois_norm_device", "host_resize_rois", "host_resize_rois_norm",
                 "hip_resize_rois_yuv_rgb_device", "hip_resize_rois_yuv_norm_device", "host_resize_rois_yuv_rgb",
                 "host_resize_rois_yuv_norm"):
        twin = name.replace("rois_yuv", "rois_yuv_fit") if "yuv" in name else name.replace("rois", "rois_fit")
        getattr(L, "iqo_" + twin).argtypes = getattr(L, "iqo_" + name).argtypes + fit
    L.iqo_host_roi_fit_arena_stats.argtypes = L.iqo_host_roi_arena_stats.argtypes + fit[:1]
    L.iqo_host_roi_yuv_fit_arena_stats.argtypes = L.iqo_host_roi_yuv_arena_stats.argtypes + fit[:1]
    L.iqo_host_fit_rect.argtypes = [ctypes.c_int, _c_sz, _c_sz, _c_sz, _c_sz, ctypes.POINTER(RoiRect)]
    L.iqo_host_roi_fit_box_layout.argtypes = roi_host + [_c_sz, _c_sz, ctypes.POINTER(RoiRect),
                                                         ctypes.POINTER(RoiFitBoxLayout)]
    L.iqo_host_roi_yuv_fit_box_layout.argtypes = roi_host + [_c_sz, _c_sz, ctypes.POINTER(RoiRect),
                                                             ctypes.POINTER(RoiYuvFitBoxLayout)]
    L.iqo_hip_copy_frames.argtypes = [_vp, ctypes.c_int, _c_sz, _vp, ctypes.c_int, _c_sz, _c_sz, _c_sz, _vp,
                                      ctypes.POINTER(ctypes.c_int)]
    L.iqo_hip_ipc_export.argtypes = [_vp, ctypes.POINTER(IpcHandle)]
    L.iqo_hip_ipc_open.argtypes = [ctypes.POINTER(IpcHandle), ctypes.c_int, ctypes.POINTER(_vp)]
    L.iqo_hip_ipc_close.argtypes = [_vp, ctypes.POINTER(IpcHandle)]
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise IqoError("%s: %s (%d)" % (what, lib().iqo_hip_strerror(rc).decode(), rc))


def available():
    """Number of usable gfx950 devices."""
    return int(lib().iqo_hip_available())


def copy_frames(dst, dst_device, dst_frame_st, src, src_device, src_frame_st, bytes_per_frame, n_frames,
                stream=None):
    """iqo_hip_copy_frames: n_frames blocks between devices (device < 0 = host).  Returns the
    route taken (COPY_PATHS)."""
    path = ctypes.c_int(-1)
    _check(lib().iqo_hip_copy_frames(_ptr(dst), dst_device, dst_frame_st, _ptr(src), src_device, src_frame_st,
                                     bytes_per_frame, n_frames, _stream_ptr(stream), ctypes.byref(path)),
           "copy_frames")
    return path.value


def ipc_export(ptr):
    """Exportable handle (bytes) of a device buffer for another process (one process per GPU)."""
    h = IpcHandle()
    _check(lib().iqo_hip_ipc_export(_ptr(ptr), ctypes.byref(h)), "ipc_export")
    return bytes(ctypes.string_at(ctypes.addressof(h), ctypes.sizeof(h)))


def ipc_open(handle_bytes, device):
    """Open another process's exported buffer on `device`; returns (address, handle)."""
    h = IpcHandle.from_buffer_copy(handle_bytes)
    p = _vp()
    _check(lib().iqo_hip_ipc_open(ctypes.byref(h), device, ctypes.byref(p)), "ipc_open")
    return p.value, h


def ipc_close(addr, h):
    _check(lib().iqo_hip_ipc_close(addr, ctypes.byref(h)), "ipc_close")


def host_tables(method, degree, srcW, srcH, dstW, dstH, pxScale, axis):
    """Quantised coefficient table (phases x taps) the plan uploads -- host only, no GPU."""
    L = lib()
    nt, npz = ctypes.c_int(), ctypes.c_int()
    total = L.iqo_host_tables(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale, axis,
                              ctypes.byref(nt), ctypes.byref(npz), None, 0)
    if total < 0:
        raise IqoError("invalid table request")
    buf = (ctypes.c_int32 * max(1, total))()
    L.iqo_host_tables(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale, axis,
                      ctypes.byref(nt), ctypes.byref(npz), buf, total)
    rows = [list(buf[q * nt.value:(q + 1) * nt.value]) for q in range(npz.value)]
    return rows


def host_band_src_rows(method, degree, srcW, srcH, dstW, dstH, pxScale, dstRow0, dstRows):
    """Source-row window (srcRow0, srcRows) read by output rows [dstRow0, dstRow0+dstRows) -- host only."""
    a, b = _c_sz(), _c_sz()
    _check(lib().iqo_host_band_src_rows(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale, dstRow0, dstRows,
                                        ctypes.byref(a), ctypes.byref(b)), "host_band_src_rows")
    return a.value, b.value


def host_kernel_for(method, degree, srcW, srcH, dstW, dstH, pxScale=1, src_align=16, dst_align=16):
    """Kernel family of a full-frame device call whose source / destination base and strides are
    multiples of src_align / dst_align bytes (powers of two, 1..16) and of nothing larger -- host
    only, no GPU."""
    k = lib().iqo_host_kernel_for_layout(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale, src_align,
                                         dst_align)
    if k < 0:
        raise IqoError("invalid plan request")
    return KERNELS[k]


def host_instance_for(method, degree, srcW, srcH, dstW, dstH, pxScale=1, options=(), src_align=16, dst_align=16):
    """The template instantiation a full-frame call of this shape runs after `options` ((key, value) pairs,
    applied as set_option applies them) with the given alignments, as {"kernel": name, parameter: value, ...}
    with the parameters that are not 0 -- host only, no GPU."""
    opts = (_Option * max(1, len(options)))(*[_Option(k.encode(), int(v)) for k, v in options])
    d = Instance()
    _check(lib().iqo_host_instance_for(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale, opts, len(options),
                                       src_align, dst_align, ctypes.byref(d)), "host_instance_for")
    return _instance_dict(d)


def host_launch_grid(method, degree, srcW, srcH, dstW, dstH, n_frames, pxScale=1, channels=1, options=()):
    """The grid of the first launch of a full-frame call of n_frames frames of this shape after `options`, as a
    dict of iqo_hip_launch_grid's fields with the family and the map by name -- host only, no GPU."""
    opts = (_Option * max(1, len(options)))(*[_Option(k.encode(), int(v)) for k, v in options])
    d = LaunchGrid()
    _check(lib().iqo_host_launch_grid(_METHODS[method], degree, channels, srcW, srcH, dstW, dstH, pxScale, opts,
                                      len(options), n_frames, ctypes.byref(d)), "host_launch_grid")
    return _grid_dict(d)


def host_instances(kernel):
    """Every instantiation of a kernel family (a KERNELS name), in the library's table order -- host only."""
    family = {v: k for k, v in KERNELS.items()}[kernel]
    out = []
    for i in range(lib().iqo_host_instance_count(family)):
        d = Instance()
        _check(lib().iqo_host_instance_at(family, i, ctypes.byref(d)), "host_instances")
        out.append(_instance_dict(d))
    return out


class LayoutLimits(ctypes.Structure):
    """iqo_hip_layout_limits: the largest accepted spans and row strides of a kernel family, 0 = unlimited."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("srcSpanMax", "dstSpanMax", "srcStMax", "dstStMax")]


DROP_OFFSET = 0x7ff00000  # iqo_hip.h IQO_HIP_DROP_OFFSET


def host_layout_limits(kernel):
    """(srcSpanMax, dstSpanMax, srcStMax, dstStMax) of a kernel family (a KERNELS name), 0 = unlimited: the
    table the launch functions test a layout against -- host only, no GPU."""
    family = {v: k for k, v in KERNELS.items()}[kernel]
    f = lib().iqo_host_layout_limits
    f.argtypes = [ctypes.c_int, ctypes.POINTER(LayoutLimits)]
    m = LayoutLimits()
    _check(f(family, ctypes.byref(m)), "host_layout_limits")
    return (m.srcSpanMax, m.dstSpanMax, m.srcStMax, m.dstStMax)


def host_lanczos_yfold(method, degree, srcW, srcH, dstW, dstH, pxScale=1):
    """True when a call of this shape runs the block-shared Lanczos 2:1 streamer with the folded vertical
    pass (its own Y table has an outer tap twice its neighbour) -- host only, no GPU."""
    f = lib().iqo_host_lanczos_yfold  # (bound here: an A/B build of an older commit loads without it)
    f.argtypes = lib().iqo_host_kernel_for.argtypes
    k = f(_METHODS[method], degree, srcW, srcH, dstW, dstH, pxScale)
    if k < 0:
        raise IqoError("invalid plan request")
    return bool(k)


def host_packed_kernel_for(method, degree, channels, srcW, srcH, dstW, dstH, pxScale=1):
    """Kernel family of a packed plan with `channels` bytes per pixel -- host only, no GPU."""
    k = lib().iqo_host_packed_kernel_for(_METHODS[method], degree, channels, srcW, srcH, dstW, dstH, pxScale)
    if k < 0:
        raise IqoError("invalid packed plan request")
    return KERNELS[k]


def host_yuv420_fused(method, degree, srcW, srcH, dstW, dstH):
    """Fused instantiation (YUV420_FUSED label) an I420 call of this shape runs with default options and an
    aligned layout, "none" when it goes plane by plane -- host only, no GPU."""
    k = lib().iqo_host_yuv420_fused(_METHODS[method], degree, srcW, srcH, dstW, dstH)
    if k < 0:
        raise IqoError("invalid yuv420 plan request")
    return YUV420_FUSED[k]


def _standard(standard):
    """IQO_CS_* of a name in COLOR_STANDARDS or of the integer itself."""
    if isinstance(standard, str):
        if standard not in COLOR_STANDARDS:
            raise IqoError("standard must be one of %s" % ", ".join(sorted(COLOR_STANDARDS)))
        return COLOR_STANDARDS[standard]
    return int(standard)


def _chroma(chroma):
    """IQO_CHROMA_* of a name in CHROMA_MODES."""
    if not isinstance(chroma, str) or chroma not in CHROMA_MODES:
        raise IqoError("chroma must be one of %s" % ", ".join(sorted(CHROMA_MODES)))
    return CHROMA_MODES[chroma]


def yuv_rgb_workspace_bytes(dstW, dstH, nFrames, chroma="replicate"):
    """Bytes of device workspace the resize_rgb / resize_normalized calls of a YUV resizer in chroma mode
    `chroma` need -- host only."""
    return int(lib().iqo_hip_yuv_rgb_workspace_bytes_chroma(dstW, dstH, nFrames, _chroma(chroma)))


def host_chroma_full_kernel(method, degree, srcW, srcH, dstW, dstH, layout="nv12"):
    """Kernel family of the full-grid chroma plan (srcW/2 x srcH/2 -> dstW x dstH, pxScale 1) of a YUV resizer
    with chroma="full": Nv12Resizer's 2-channel packed plan (layout "nv12") or Yuv420Resizer's planar plan
    ("i420") -- host only, no GPU.  Raises IqoError, with the status chroma="full" would fail with, for a
    shape that has no such plan."""
    if layout not in ("nv12", "i420"):
        raise IqoError("layout must be nv12 or i420")
    k = lib().iqo_host_yuv_chroma_full_kernel(_METHODS[method], degree, srcW, srcH, dstW, dstH, int(layout == "nv12"))
    _check(k if k < 0 else 0, "host_chroma_full_kernel")
    return KERNELS[k]


def host_yuv_to_rgb(standard, y, u, v):
    """The library's integer YUV -> RGB formula (include/iqo_hip.h, IQO_CS_*) on numpy uint8 arrays of one
    shape, in plain C++ on the host -- no GPU.  Returns uint8 [..., 3] (R, G, B)."""
    import numpy as np
    y, u, v = (np.ascontiguousarray(a, dtype=np.uint8) for a in (y, u, v))
    if not (y.shape == u.shape == v.shape):
        raise IqoError("y, u and v must have one shape")
    rgb = np.empty(y.shape + (3,), np.uint8)
    _check(lib().iqo_host_yuv_to_rgb(_standard(standard), y.size, _ptr(y), _ptr(u), _ptr(v), _ptr(rgb)),
           "host_yuv_to_rgb")
    return rgb


def rgb_yuv_workspace_bytes(dstW, dstH, channels, nFrames):
    """Bytes of device workspace the resize_nv12 / resize_i420 calls of a packed resizer with `channels` (3 or
    4) bytes per pixel need -- host only."""
    return int(lib().iqo_hip_rgb_yuv_workspace_bytes(dstW, dstH, channels, nFrames))


def planes_norm_workspace_bytes(dstW, dstH, srcPlanes, nFrames):
    """Bytes of device workspace a resize_planes_normalized / resize_luma_normalized call with `srcPlanes`
    (1..4) source planes per frame needs -- host only."""
    return int(lib().iqo_hip_planes_norm_workspace_bytes(dstW, dstH, srcPlanes, nFrames))


def host_rgb_to_yuv(standard, rgb):
    """The library's integer RGB -> YUV formula in its 4:4:4 form (include/iqo_hip.h, IQO_CS_*) on a numpy
    uint8 array [..., 3] (R, G, B), in plain C++ on the host -- no GPU.  Returns (y, u, v), uint8 [...]."""
    import numpy as np
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise IqoError("rgb must be [..., 3]")
    y, u, v = (np.empty(rgb.shape[:-1], np.uint8) for _ in range(3))
    _check(lib().iqo_host_rgb_to_yuv(_standard(standard), y.size, _ptr(rgb), _ptr(y), _ptr(u), _ptr(v)),
           "host_rgb_to_yuv")
    return y, u, v


def host_rgb_to_yuv420(standard, rgb):
    """The 4:2:0 form on one image, numpy uint8 [h, w, 3] (R, G, B): Y per pixel, U and V once per 2 x 2 block
    on the block's sums -- no GPU.  Returns (y [h, w], u [h/2, w/2], v [h/2, w/2])."""
    import numpy as np
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise IqoError("rgb must be [h, w, 3]")
    h, w = rgb.shape[:2]
    y = np.empty((h, w), np.uint8)
    u, v = (np.empty((h // 2, w // 2), np.uint8) for _ in range(2))
    _check(lib().iqo_host_rgb_to_yuv420(_standard(standard), w, h, _ptr(rgb), _ptr(y), _ptr(u), _ptr(v)),
           "host_rgb_to_yuv420")
    return y, u, v


def _roi_array(boxes):
    """(frame, x, y, w, h[, flip]) tuples -> a ctypes array of iqo_hip_roi."""
    arr = (Roi * max(1, len(boxes)))()
    for i, b in enumerate(boxes):
        if len(b) not in (5, 6):
            raise IqoError("box %d: expected (frame, x, y, w, h) or (frame, x, y, w, h, flip)" % i)
        arr[i] = Roi(int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(b[4]), int(b[5]) if len(b) == 6 else 0)
    return arr


def _check_rois(rc, bad, boxes, what, where=None):
    if rc != 0:
        if where is None:
            where = " (box %d: %s)" % (bad.value, tuple(boxes[bad.value])) if 0 <= bad.value < len(boxes) else ""
        err = IqoError("%s: %s (%d)%s" % (what, lib().iqo_hip_strerror(rc).decode(), rc, where))
        err.status, err.bad_roi = rc, bad.value  # IQO_HIP_E*, the first offending box (-1: the call itself)
        raise err


def fit_rects(boxes, dstW, dstH, mode="letterbox"):
    """iqo_host_fit_rect per box: the rectangles [(x, y, w, h)] of a dstW x dstH output that boxes (frame, x, y, w,
    h[, flip]) go to with their aspect ratio kept ("letterbox": centred; "letterbox-topleft"; "stretch": the whole
    output).  A point (px, py) of output i lies at x + (px - rx + 0.5) * w / rw - 0.5 of the frame (y alike)."""
    if mode not in FIT_MODES:
        raise IqoError("fit must be one of %s" % ", ".join(sorted(FIT_MODES)))
    out, r = [], RoiRect()
    for i, b in enumerate(boxes):
        rc = lib().iqo_host_fit_rect(FIT_MODES[mode], max(int(b[3]), 0), max(int(b[4]), 0), dstW, dstH, ctypes.byref(r))
        if rc != 0:
            raise IqoError("fit_rects: box %d %s into %d x %d: %s (%d)" % (i, tuple(b), dstW, dstH,
                                                                         lib().iqo_hip_strerror(rc).decode(), rc))
        out.append((r.x, r.y, r.w, r.h))
    return out


def _fit_args(boxes, dstW, dstH, rects, fit, pad):
    """() for a stretch call (no rects, no fit, pad 0), or the two trailing arguments of a fit entry.  A nonzero pad
    alone selects the fit entry with no rectangles: the same output as the stretch call, by the fit arena and kernel."""
    import operator
    if rects is not None and fit is not None:
        raise IqoError("give rects or fit, not both")
    try:
        pad = tuple(operator.index(v) for v in pad) if hasattr(pad, "__len__") else (operator.index(pad),) * 4
    except TypeError:
        raise IqoError("pad: an int or up to 4 ints, 0 .. 255")
    if len(pad) > 4 or any(not 0 <= v <= 255 for v in pad):
        raise IqoError("pad: an int or up to 4 ints, 0 .. 255")
    if rects is None and fit is None and not any(pad):
        return ()
    if fit is not None:
        if fit not in ("letterbox", "letterbox-topleft"):
            raise IqoError("fit must be letterbox or letterbox-topleft")
        rects = fit_rects(boxes, dstW, dstH, fit)
    arr = None
    if rects is not None:
        rects = [tuple(int(v) for v in r) for r in rects]
        if len(rects) != len(boxes) or any(len(r) != 4 for r in rects):
            raise IqoError("rects: one (x, y, w, h) per box")
        arr = (RoiRect * max(1, len(rects)))(*[RoiRect(*r) for r in rects])
    return (arr, (ctypes.c_ubyte * 4)(*(pad + (0,) * (4 - len(pad)))))


def _norm_of(C, scale, bias, order, code):
    order = tuple(range(C)) if order is None else tuple(int(c) for c in order)
    scale, bias = tuple(float(v) for v in scale), tuple(float(v) for v in bias)
    planes = len(order)
    if not 1 <= planes <= 4 or len(scale) != planes or len(bias) != planes:
        raise IqoError("order, scale and bias must have the same length, 1..4 (one entry per output plane)")
    n = Norm(code, planes)
    for i in range(planes):
        n.order[i], n.scale[i], n.bias[i] = order[i], scale[i], bias[i]
    return n, planes


def _host_roi_out_u8(shape, C, out):
    """`out`, or a new array: uint8 of `shape` with contiguous pixels."""
    import numpy as np
    if out is None:
        out = np.zeros(shape, np.uint8)
    if out.dtype != np.uint8 or out.shape != shape or (shape[0] and (out.strides[2] != C or
                                                                     (len(shape) == 4 and out.strides[3] != 1))):
        raise IqoError("out must be a uint8 array %s with contiguous pixels" % (shape,))
    return out


def _host_roi_out_norm(C, scale, bias, order, dtype, N, dstH, dstW, out):
    """(iqo_hip_norm, `out` or a new array [N, planes, dstH, dstW] of `dtype` with unit column stride)."""
    import numpy as np
    codes = {"float32": (OUT_F32, np.float32), "float16": (OUT_F16, np.float16), "bfloat16": (OUT_BF16, np.uint16)}
    code, np_dtype = codes[dtype or "float32"]
    n, planes = _norm_of(C, scale, bias, order, code)
    shape = (N, planes, dstH, dstW)
    if out is None:
        out = np.zeros(shape, np_dtype)
    if out.dtype != np_dtype or out.shape != shape or (N and out.strides[3] != out.itemsize):
        raise IqoError("out must be a %s array %s with unit column stride" % (np_dtype.__name__, shape))
    return n, out


def _host_arena_stats(entry, method, degree, variant, dstW, dstH, boxes, nFrames, frameW, frameH, rects=None, fit=None):
    m = _METHODS[method] if isinstance(method, str) else int(method)
    boxes = [tuple(b) for b in boxes]
    st, bad = RoiArenaStats(), ctypes.c_int(-1)
    tail = _fit_args(boxes, dstW, dstH, rects, fit, 0)[:1]
    if tail:
        entry = entry.replace("_arena", "_fit_arena")
    rc = getattr(lib(), "iqo_" + entry)(m, degree, variant, dstW, dstH, len(boxes), _roi_array(boxes), nFrames, frameW,
                                        frameH, ctypes.byref(st), ctypes.byref(bad), *tail)
    _check_rois(rc, bad, boxes, entry)
    return {"arena_bytes": st.arenaBytes, "x_tables": st.xTables, "y_tables": st.yTables, "workgroups": st.workgroups,
            "lds_bytes": st.ldsBytes, "record_bytes": st.recordBytes}


def host_resize_rois(method, degree, dstW, dstH, src, boxes, scale=None, bias=None, dtype=None, order=None, out=None,
                     rects=None, fit=None, pad=0):
    """iqo_host_resize_rois / iqo_host_resize_rois_norm on numpy arrays (no GPU): the CPU twin of
    RoiResizer.resize_rois and, with scale / bias, of resize_rois_normalized.  src: uint8 [F, H, W] or
    [F, H, W, C] (row and frame strides free, pixel bytes contiguous).  Returns uint8 [N, dstH, dstW(, C)], or
    [N, planes, dstH, dstW] of dtype "float32", "float16" (numpy arrays of that type) or "bfloat16" (uint16 bit
    patterns).  rects / fit / pad: the fit twins (iqo_host_resize_rois_fit / _fit_norm), as RoiResizer.resize_rois."""
    import numpy as np
    m = _METHODS[method] if isinstance(method, str) else int(method)
    if src.dtype != np.uint8 or src.ndim not in (3, 4):
        raise IqoError("expected a uint8 array [F, H, W] or [F, H, W, C]")
    C = 1 if src.ndim == 3 else src.shape[3]
    if src.strides[2] != C or (src.ndim == 4 and src.strides[3] != 1) or min(src.strides[0], src.strides[1]) < 1:
        src = np.ascontiguousarray(src)
    F, H, W = src.shape[:3]
    boxes = [tuple(b) for b in boxes]
    arr, bad, N = _roi_array(boxes), ctypes.c_int(-1), len(boxes)
    tail = _fit_args(boxes, dstW, dstH, rects, fit, pad)
    sfx = "_fit" if tail else ""
    head = (m, degree, C, dstW, dstH, N, arr, F, W, H, src.strides[1], src.strides[0], src.ctypes.data)
    if scale is None:
        out = _host_roi_out_u8((N, dstH, dstW) if src.ndim == 3 else (N, dstH, dstW, C), C, out)
        if N == 0:  # (numpy gives an empty array no usable strides)
            return out
        rc = getattr(lib(), "iqo_host_resize_rois" + sfx)(*head, out.strides[1], out.strides[0], out.ctypes.data,
                                                          ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "host_resize_rois")
        return out
    n, out = _host_roi_out_norm(C, scale, bias, order, dtype, N, dstH, dstW, out)
    if N == 0:
        return out
    rc = getattr(lib(), "iqo_host_resize_rois%s_norm" % sfx)(*head, ctypes.byref(n), out.strides[2], out.strides[1],
                                                             out.strides[0], out.ctypes.data, ctypes.byref(bad), *tail)
    _check_rois(rc, bad, boxes, "host_resize_rois")
    return out


def host_roi_arena_stats(method, degree, dstW, dstH, channels, boxes, nFrames, frameW, frameH, rects=None, fit=None):
    """iqo_host_roi_arena_stats: {"arena_bytes", "x_tables", "y_tables", "workgroups", "lds_bytes", "record_bytes"}
    of the call's arena, without a GPU.  With rects or fit: of the fit call's (iqo_host_roi_fit_arena_stats)."""
    return _host_arena_stats("host_roi_arena_stats", method, degree, channels, dstW, dstH, boxes, nFrames, frameW, frameH,
                             rects, fit)


def _fit_layout_dict(d, bl):
    d.update({"pad_above": bl.padAbove, "pad_below": bl.padBelow, "pad_rows": bl.padRows})
    return d


def host_roi_fit_box_layout(method, degree, channels, dstW, dstH, w, h, rect=None):
    """iqo_host_roi_fit_box_layout: host_roi_box_layout of (w, h) -> the rectangle's (iw, ih), and "pad_above",
    "pad_below" (pad workgroups above and below rectangle (x, y, iw, ih); None: the whole output) and "pad_rows" (the
    canvas rows one of them writes, at most)."""
    m = _METHODS[method] if isinstance(method, str) else int(method)
    bl, r = RoiFitBoxLayout(), None if rect is None else RoiRect(*[int(v) for v in rect])
    rc = lib().iqo_host_roi_fit_box_layout(m, degree, channels, dstW, dstH, w, h, r, ctypes.byref(bl))
    _check_rois(rc, ctypes.c_int(-1), (), "host_roi_fit_box_layout", " (box %d x %d into %s)" % (w, h, rect))
    b = bl.box
    return _fit_layout_dict({"rows": b.rows, "workgroups": b.workgroups, "lds_bytes": b.ldsBytes, "nYp": b.nYp, "NP": b.np,
                             "pitchDw": b.pitchDw}, bl)


def host_roi_box_layout(method, degree, channels, dstW, dstH, w, h):
    """iqo_host_roi_box_layout: {"rows", "workgroups", "lds_bytes", "nYp", "NP", "pitchDw"} the layout of a call
    decides for one box of w x h pixels, without a GPU."""
    m = _METHODS[method] if isinstance(method, str) else int(method)
    bl = RoiBoxLayout()
    rc = lib().iqo_host_roi_box_layout(m, degree, channels, dstW, dstH, w, h, ctypes.byref(bl))
    _check_rois(rc, ctypes.c_int(-1), (), "host_roi_box_layout", " (box %d x %d)" % (w, h))  # (names no box index)
    return {"rows": bl.rows, "workgroups": bl.workgroups, "lds_bytes": bl.ldsBytes, "nYp": bl.nYp, "NP": bl.np,
            "pitchDw": bl.pitchDw}


def _roi_layout(layout):
    if layout not in ROI_LAYOUTS:
        raise IqoError("layout must be nv12 or i420")
    return ROI_LAYOUTS[layout]


def _yuv_planes(layout, base, frameW, frameH):
    """(srcStY, srcStUV, Y, U or UV, V or None) of the tight frame layout at address `base`."""
    if frameW < 2 or frameH < 2 or frameW % 2 or frameH % 2:
        return frameW, frameW, base, base, (None if layout == "nv12" else base)  # (the call rejects the size)
    n = frameW * frameH
    if layout == "nv12":
        return frameW, frameW, base, base + n, None
    return frameW, frameW // 2, base, base + n, base + n + n // 4


def _rgb_order(order):
    if order not in RGB_ORDERS:
        raise IqoError("order must be one of %s" % ", ".join(sorted(RGB_ORDERS)))
    o4 = RGB_ORDERS[order]
    return len(o4), (ctypes.c_int * 4)(*(o4 + (0,) * (4 - len(o4))))


def host_resize_rois_yuv(method, degree, dstW, dstH, src, boxes, frameW, frameH, layout="nv12", standard="bt709",
                         order="rgb", scale=None, bias=None, dtype=None, planes=(0, 1, 2), out=None, rects=None, fit=None,
                         pad=0):
    """iqo_host_resize_rois_yuv_rgb / _norm on numpy arrays (no GPU): the CPU twin of YuvRoiResizer.resize_rois_rgb
    and, with scale / bias, of resize_rois_normalized (`planes`: its order).  src: uint8 [F, frameW*frameH*3/2], the
    tight NV12 / I420 frames (unit byte stride; the frame stride is free).  Returns uint8 [N, dstH, dstW, 3|4], or
    [N, planes, dstH, dstW] of "float32", "float16" or "bfloat16" (uint16 bit patterns).  rects / fit / pad: the fit
    twins (iqo_host_resize_rois_yuv_fit_rgb / _fit_norm), as YuvRoiResizer.resize_rois_rgb; pad is (R, G, B)."""
    import numpy as np
    m = _METHODS[method] if isinstance(method, str) else int(method)
    lay, cs = _roi_layout(layout), _standard(standard)
    if src.dtype != np.uint8 or src.ndim != 2 or src.shape[1] != frameW * frameH * 3 // 2:
        raise IqoError("expected a uint8 array [F, %d]" % (frameW * frameH * 3 // 2))
    if src.strides[1] != 1 or src.strides[0] < 1:
        src = np.ascontiguousarray(src)
    boxes = [tuple(b) for b in boxes]
    arr, bad, N = _roi_array(boxes), ctypes.c_int(-1), len(boxes)
    tail = _fit_args(boxes, dstW, dstH, rects, fit, pad)
    sfx = "_fit" if tail else ""
    stY, stUV, y, u, v = _yuv_planes(layout, src.ctypes.data, frameW, frameH)
    head = (m, degree, lay, dstW, dstH, N, arr, src.shape[0], frameW, frameH, stY, stUV, src.strides[0], y, u, v, cs)
    if scale is None:
        C, o4 = _rgb_order(order)
        out = _host_roi_out_u8((N, dstH, dstW, C), C, out)
        if N == 0:
            return out
        rc = getattr(lib(), "iqo_host_resize_rois_yuv%s_rgb" % sfx)(*head, C, o4, out.strides[1], out.strides[0],
                                                                    out.ctypes.data, ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "host_resize_rois_yuv")
        return out
    n, out = _host_roi_out_norm(3, scale, bias, planes, dtype, N, dstH, dstW, out)
    if N == 0:
        return out
    rc = getattr(lib(), "iqo_host_resize_rois_yuv%s_norm" % sfx)(*head, ctypes.byref(n), out.strides[2], out.strides[1],
                                                                 out.strides[0], out.ctypes.data, ctypes.byref(bad), *tail)
    _check_rois(rc, bad, boxes, "host_resize_rois_yuv")
    return out


def host_roi_yuv_arena_stats(method, degree, dstW, dstH, layout, boxes, nFrames, frameW, frameH, rects=None, fit=None):
    """iqo_host_roi_yuv_arena_stats: host_roi_arena_stats of a YUV box call; "x_tables" / "y_tables" count every
    distinct table once, whether luma, chroma or both use it."""
    return _host_arena_stats("host_roi_yuv_arena_stats", method, degree, _roi_layout(layout), dstW, dstH, boxes, nFrames,
                             frameW, frameH, rects, fit)


def host_roi_yuv_fit_box_layout(method, degree, layout, dstW, dstH, w, h, rect=None):
    """iqo_host_roi_yuv_fit_box_layout: host_roi_yuv_box_layout of (w, h) -> the rectangle's (iw, ih), and the pad
    workgroups of host_roi_fit_box_layout."""
    m = _METHODS[method] if isinstance(method, str) else int(method)
    bl, r = RoiYuvFitBoxLayout(), None if rect is None else RoiRect(*[int(v) for v in rect])
    rc = lib().iqo_host_roi_yuv_fit_box_layout(m, degree, _roi_layout(layout), dstW, dstH, w, h, r, ctypes.byref(bl))
    _check_rois(rc, ctypes.c_int(-1), (), "host_roi_yuv_fit_box_layout", " (box %d x %d into %s)" % (w, h, rect))
    b = bl.box
    return _fit_layout_dict({"rows": b.rows, "workgroups": b.workgroups, "lds_bytes": b.ldsBytes, "nYp": b.nYp, "NP": b.np,
                             "pitchDw": b.pitchDw, "nYpC": b.nYpC, "NPC": b.npC, "pitchDwC": b.pitchDwC}, bl)


def host_roi_yuv_box_layout(method, degree, layout, dstW, dstH, w, h):
    """iqo_host_roi_yuv_box_layout: {"rows", "workgroups", "lds_bytes"} and {"nYp", "NP", "pitchDw"} of luma and, with
    a "C" appended, of chroma, as the layout of a call decides for one box of w x h pixels, without a GPU."""
    m = _METHODS[method] if isinstance(method, str) else int(method)
    bl = RoiYuvBoxLayout()
    rc = lib().iqo_host_roi_yuv_box_layout(m, degree, _roi_layout(layout), dstW, dstH, w, h, ctypes.byref(bl))
    _check_rois(rc, ctypes.c_int(-1), (), "host_roi_yuv_box_layout", " (box %d x %d)" % (w, h))
    return {"rows": bl.rows, "workgroups": bl.workgroups, "lds_bytes": bl.ldsBytes, "nYp": bl.nYp, "NP": bl.np,
            "pitchDw": bl.pitchDw, "nYpC": bl.nYpC, "NPC": bl.npC, "pitchDwC": bl.pitchDwC}


def _ptr(obj):
    """Raw address of a numpy array, a torch tensor or an int."""
    if isinstance(obj, int):
        return obj
    if hasattr(obj, "data_ptr"):
        return obj.data_ptr()
    if hasattr(obj, "ctypes"):
        return obj.ctypes.data
    raise TypeError("expected numpy array, torch tensor or address")


def _stream_ptr(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream  # torch.cuda.Stream on ROCm wraps a hipStream_t


def _planes_norm(r, what, plan, src4, layout, scale, bias, dtype, order, squeeze, out, stream):
    """resize_planes_normalized / resize_luma_normalized: iqo_hip_resize_planes_norm_device with the 1-channel
    plan `plan` of resizer `r`.  layout: (frames, srcPlanes, srcSt, srcPlaneSt, srcFrameSt, address) of the
    source `src4` lies on; order, scale, bias: one entry per output plane."""
    import torch
    if dtype is None:
        dtype = torch.float32
    codes = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
    if dtype not in codes:
        raise IqoError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
    frames, P, src_st, plane_st, frame_st, addr = layout
    order = tuple(int(c) for c in order)
    scale, bias = tuple(float(v) for v in scale), tuple(float(v) for v in bias)
    planes = len(order)
    if not 1 <= planes <= 4 or len(scale) != planes or len(bias) != planes:
        raise IqoError("order, scale and bias must have the same length, 1..4 (one entry per output plane)")
    if any(not 0 <= c < P for c in order):
        raise IqoError("order entries must be source planes, 0..%d" % (P - 1))
    dev = src4.device
    shape = (frames, planes, r.dstH, r.dstW)
    if out is None:
        out = torch.empty(shape[1:] if squeeze else shape, dtype=dtype, device=dev)
    o = out.unsqueeze(0) if out.dim() == 3 else out
    if (o.dtype != dtype or o.device != dev or tuple(o.shape) != shape or o.stride(3) != 1
            or o.stride(2) < r.dstW or o.stride(1) < r.dstH * o.stride(2)
            or (o.shape[0] > 1 and o.stride(0) < planes * o.stride(1))):
        raise IqoError("out must be a %s tensor [%d, %d, %d, %d] on %s with unit column stride and "
                       "non-overlapping rows, planes and frames" % ((dtype,) + shape + (dev,)))
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    n = Norm(codes[dtype], planes)
    for i in range(planes):
        n.order[i], n.scale[i], n.bias[i] = order[i], scale[i], bias[i]
    e = o.element_size()
    ws = _Resizer._yuv_workspace(r, planes_norm_workspace_bytes(r.dstW, r.dstH, P, frames), dev, stream)
    _check(lib().iqo_hip_resize_planes_norm_device(plan, frames, P, src_st, plane_st, frame_st, addr, ctypes.byref(n),
                                                   o.stride(2) * e, o.stride(1) * e, o.stride(0) * e, _ptr(o),
                                                   _ptr(ws), ws.numel(), _stream_ptr(stream)), what)
    return out


class _Resizer:
    _method = None

    def __init__(self, srcW, srcH, dstW, dstH, device=None, channels=1):
        self.srcW, self.srcH, self.dstW, self.dstH = int(srcW), int(srcH), int(dstW), int(dstH)
        self.device = 0 if device is None else int(device)
        self.channels = int(channels)  # bytes per pixel, interleaved (widths stay in pixels, strides in bytes)
        self._plan = _vp()
        if self.channels == 1:
            self._make()
        else:
            _check(lib().iqo_hip_plan_packed(self._method, getattr(self, "degree", 0), self.channels, self.srcW,
                                             self.srcH, self.dstW, self.dstH, getattr(self, "pxScale", 1), self.device,
                                             ctypes.byref(self._plan)), type(self).__name__)

    def _make(self):
        raise NotImplementedError

    def __del__(self):
        p = getattr(self, "_plan", None)
        if p and _lib is not None:
            _lib.iqo_hip_plan_destroy(p)
            self._plan = _vp()

    # -- reference entry point (host pointers, byte strides): resize(srcSt, src, dstSt, dst)
    def resize(self, srcSt, src, dstSt, dst):
        _check(lib().iqo_hip_resize(self._plan, srcSt, _ptr(src), dstSt, _ptr(dst)), "resize")

    # -- batched device-resident form (async on `stream`)
    def resize_device(self, nFrames, srcSt, srcFrameSt, src, dstSt, dstFrameSt, dst, stream=None):
        _check(lib().iqo_hip_resize_device(self._plan, nFrames, srcSt, srcFrameSt, _ptr(src), dstSt, dstFrameSt,
                                           _ptr(dst), _stream_ptr(stream)), "resize_device")

    def band_src_rows(self, dstRow0, dstRows):
        a, b = _c_sz(), _c_sz()
        _check(lib().iqo_hip_band_src_rows(self._plan, dstRow0, dstRows, ctypes.byref(a), ctypes.byref(b)),
               "band_src_rows")
        return a.value, b.value

    def resize_band(self, nFrames, dstRow0, dstRows, srcRow0, srcSt, srcFrameSt, src, dstSt, dstFrameSt, dst,
                    stream=None):
        _check(lib().iqo_hip_resize_band(self._plan, nFrames, dstRow0, dstRows, srcRow0, srcSt, srcFrameSt,
                                         _ptr(src), dstSt, dstFrameSt, _ptr(dst), _stream_ptr(stream)),
               "resize_band")

    def set_option(self, key, value):
        _check(lib().iqo_hip_plan_set_option(self._plan, key.encode(), int(value)), "set_option")

    def instance(self, src_align=16, dst_align=16):
        """The template instantiation a full-frame call runs with the plan's current options (host_instance_for's
        form)."""
        d = Instance()
        _check(lib().iqo_hip_plan_instance(self._plan, src_align, dst_align, ctypes.byref(d)), "instance")
        return _instance_dict(d)

    def launch_grid(self, n_frames, dst_row0=0, dst_rows=None):
        """The grid of the first launch of a call of n_frames frames over dst_rows output rows from dst_row0 (all
        of them by default) with the plan's current options (host_launch_grid's form)."""
        d = LaunchGrid()
        rows = self.dstH - dst_row0 if dst_rows is None else dst_rows
        _check(lib().iqo_hip_plan_launch_grid(self._plan, n_frames, dst_row0, rows, ctypes.byref(d)), "launch_grid")
        return _grid_dict(d)

    def prepare(self):
        """Upload the device tables now (before graph capture / async-only use)."""
        _check(lib().iqo_hip_plan_prepare(self._plan), "prepare")

    def describe(self):
        d = PlanDesc()
        _check(lib().iqo_hip_plan_query(self._plan, ctypes.byref(d)), "query")
        inst = Instance()  # (packed plans, and a forced prefetch depth the kernel has not: no instance)
        rc = lib().iqo_hip_plan_instance(self._plan, 16, 16, ctypes.byref(inst))
        return {"method": d.method, "device": d.device, "tapsX": d.tapsX, "tapsY": d.tapsY,
                "phasesX": d.phasesX, "phasesY": d.phasesY, "kernel": KERNELS.get(d.kernel, d.kernel),
                "bands": d.bandsPerFrame, "tile_rows": d.tileRows,
                "channels": int(lib().iqo_hip_plan_channels(self._plan)),
                "instance": _instance_dict(inst) if rc == 0 else None}

    # -- torch convenience: src [F, srcH, srcW] (or [srcH, srcW]) uint8 on the plan's device;
    #    packed plans: [F, srcH, srcW, C] (or [srcH, srcW, C])
    def resize_tensor(self, src, out=None, stream=None):
        if self.channels > 1:
            return self._resize_tensor_packed(src, out, stream)
        import torch
        squeeze = src.dim() == 2
        s = src.unsqueeze(0) if squeeze else src
        if s.dtype != torch.uint8 or not s.is_cuda or s.shape[-2:] != (self.srcH, self.srcW):
            raise IqoError("expected uint8 device tensor [F, %d, %d]" % (self.srcH, self.srcW))
        s = s.contiguous()
        if out is None:
            out = torch.empty((s.shape[0], self.dstH, self.dstW), dtype=torch.uint8, device=s.device)
        o = out.unsqueeze(0) if out.dim() == 2 else out
        if (o.dtype != torch.uint8 or o.device != s.device or tuple(o.shape) != (s.shape[0], self.dstH, self.dstW)
                or o.stride(2) != 1 or o.stride(1) < self.dstW or (o.shape[0] > 1 and o.stride(0) < self.dstH * o.stride(1))):
            raise IqoError("out must be a uint8 tensor [%d, %d, %d] on %s with unit column stride and "
                           "non-overlapping rows and frames" % (s.shape[0], self.dstH, self.dstW, s.device))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        self.resize_device(s.shape[0], s.stride(1), s.stride(0), s, o.stride(1), o.stride(0), o, stream)
        return out[0] if squeeze else out


    def _resize_tensor_packed(self, src, out, stream):
        import torch
        C = self.channels
        squeeze = src.dim() == 3
        s = src.unsqueeze(0) if squeeze else src
        if s.dtype != torch.uint8 or not s.is_cuda or s.dim() != 4 or tuple(s.shape[1:]) != (self.srcH, self.srcW, C):
            raise IqoError("expected uint8 device tensor [F, %d, %d, %d]" % (self.srcH, self.srcW, C))
        s = s.contiguous()
        shape = (s.shape[0], self.dstH, self.dstW, C)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=s.device)
        o = out.unsqueeze(0) if out.dim() == 3 else out
        if (o.dtype != torch.uint8 or o.device != s.device or tuple(o.shape) != shape or o.stride(3) != 1
                or o.stride(2) != C or o.stride(1) < self.dstW * C
                or (o.shape[0] > 1 and o.stride(0) < self.dstH * o.stride(1))):
            raise IqoError("out must be a uint8 tensor [%d, %d, %d, %d] on %s with interleaved channels and "
                           "non-overlapping rows and frames" % (shape + (s.device,)))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        self.resize_device(s.shape[0], s.stride(1), s.stride(0), s, o.stride(1), o.stride(0), o, stream)
        return out[0] if squeeze else out

    # -- packed plans straight to a model's input: planar float planes of (byte * scale + bias)
    def resize_normalized(self, src, scale, bias, dtype=None, order=None, out=None, stream=None):
        """iqo_hip_resize_device_norm on torch tensors.  src: [F, srcH, srcW, C] (or [srcH, srcW, C]) uint8 on
        the plan's device.  Returns [F, planes, dstH, dstW] (or [planes, dstH, dstW]) of `dtype` (float32,
        float16 or bfloat16): plane p is float32(byte of channel order[p]) * scale[p] + bias[p], each
        operation rounded to float32, then rounded to `dtype`.  planes = len(order), or C with the identity
        order.  `out` may be a strided view with unit column stride and non-overlapping rows, planes and
        frames; it is returned."""
        import torch
        if dtype is None:
            dtype = torch.float32
        C = self.channels
        if C < 2:
            raise IqoError("resize_normalized needs a packed resizer (channels 2..4)")
        codes = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
        if dtype not in codes:
            raise IqoError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
        order = tuple(range(C)) if order is None else tuple(int(c) for c in order)
        scale, bias = tuple(float(v) for v in scale), tuple(float(v) for v in bias)
        planes = len(order)
        if not 1 <= planes <= 4 or len(scale) != planes or len(bias) != planes:
            raise IqoError("order, scale and bias must have the same length, 1..4 (one entry per output plane)")
        squeeze = src.dim() == 3
        s = src.unsqueeze(0) if squeeze else src
        if s.dtype != torch.uint8 or not s.is_cuda or s.dim() != 4 or tuple(s.shape[1:]) != (self.srcH, self.srcW, C):
            raise IqoError("expected uint8 device tensor [F, %d, %d, %d]" % (self.srcH, self.srcW, C))
        s = s.contiguous()
        shape = (s.shape[0], planes, self.dstH, self.dstW)
        if out is None:
            out = torch.empty(shape[1:] if squeeze else shape, dtype=dtype, device=s.device)
        o = out.unsqueeze(0) if out.dim() == 3 else out
        if (o.dtype != dtype or o.device != s.device or tuple(o.shape) != shape or o.stride(3) != 1
                or o.stride(2) < self.dstW or o.stride(1) < self.dstH * o.stride(2)
                or (o.shape[0] > 1 and o.stride(0) < planes * o.stride(1))):
            raise IqoError("out must be a %s tensor [%d, %d, %d, %d] on %s with unit column stride and "
                           "non-overlapping rows, planes and frames" % ((dtype,) + shape + (s.device,)))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        n = Norm(codes[dtype], planes)
        for i in range(planes):
            n.order[i], n.scale[i], n.bias[i] = order[i], scale[i], bias[i]
        e = o.element_size()
        _check(lib().iqo_hip_resize_device_norm(self._plan, s.shape[0], s.stride(1), s.stride(0), _ptr(s),
                                                ctypes.byref(n), o.stride(2) * e, o.stride(1) * e, o.stride(0) * e,
                                                _ptr(o), _stream_ptr(stream)), "resize_normalized")
        return out

    # -- planar plans straight to a model's input: CHW bytes in, planar float planes out
    def resize_planes_normalized(self, src, scale, bias, dtype=None, order=None, out=None, stream=None):
        """iqo_hip_resize_planes_norm_device on torch tensors, for 1-channel resizers.  src: [F, P, srcH, srcW]
        (or [P, srcH, srcW]) uint8 on the plan's device, P in 1..4: planar RGB from an image decoder, grey
        images, a crop or a channel slice of either.  A strided view is read where it lies, without a copy, as
        long as its column stride is 1 and its row, plane and frame strides are positive (.contiguous() is
        taken otherwise).  Returns / fills out [F, planes, dstH, dstW] (or [planes, dstH, dstW]) of `dtype`
        (float32, float16 or bfloat16): plane p is float32(byte of source plane order[p]) * scale[p] + bias[p],
        each operation rounded to float32, then rounded to `dtype` -- what resize_tensor on the planes followed
        by those two torch operations gives, bit for bit.  planes = len(order), or P with the identity order;
        order may repeat, drop and permute source planes, and a plane it does not name is not resized.  `out`
        may be a strided view with unit column stride and non-overlapping rows, planes and frames; it is
        returned."""
        import torch
        if self.channels > 1:
            raise IqoError("resize_planes_normalized needs a 1-channel resizer; packed resizers have "
                           "resize_normalized")
        squeeze = src.dim() == 3
        s = src.unsqueeze(0) if squeeze else src
        if (s.dtype != torch.uint8 or not s.is_cuda or s.dim() != 4 or not 1 <= s.shape[1] <= 4
                or tuple(s.shape[2:]) != (self.srcH, self.srcW)):
            raise IqoError("expected uint8 device tensor [F, P, %d, %d] with P in 1..4" % (self.srcH, self.srcW))
        if s.stride(3) != 1 or min(s.stride(0), s.stride(1), s.stride(2)) < 1:
            s = s.contiguous()
        P = s.shape[1]
        layout = (s.shape[0], P, s.stride(2), s.stride(1), s.stride(0), s.data_ptr())
        return _planes_norm(self, "resize_planes_normalized", self._plan, s, layout, scale, bias, dtype,
                            tuple(range(P)) if order is None else order, squeeze, out, stream)

    # -- packed RGB(A) plans straight to an encoder's input: a Y plane and 4:2:0 chroma
    def _yuv_workspace(self, nbytes, device, stream):
        """The device workspace of a call on `stream`: one per (device, stream), kept on the resizer and grown
        when a batch needs more (_YuvToRgb._workspace has the reasons)."""
        import torch
        cache = self.__dict__.setdefault("_ws", {})
        key = (device, _stream_ptr(stream))
        ws = cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = cache[key] = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        if hasattr(stream, "cuda_stream"):
            ws.record_stream(stream)
        return ws

    def _resize_yuv(self, nv12, src, standard, order, out, stream):
        import torch
        what = "resize_nv12" if nv12 else "resize_i420"
        C = self.channels
        if C not in (3, 4):
            raise IqoError("%s needs a packed resizer with 3 or 4 channels" % what)
        if not isinstance(order, str) or order not in SOURCE_ORDERS:
            raise IqoError("order must be one of %s" % ", ".join(sorted(SOURCE_ORDERS)))
        cs = _standard(standard)
        squeeze = src.dim() == 3
        s = src.unsqueeze(0) if squeeze else src
        if s.dtype != torch.uint8 or not s.is_cuda or s.dim() != 4 or tuple(s.shape[1:]) != (self.srcH, self.srcW, C):
            raise IqoError("expected uint8 device tensor [F, %d, %d, %d]" % (self.srcH, self.srcW, C))
        s = s.contiguous()
        dw, dh = self.dstW, self.dstH
        cw, ch = dw // 2, dh // 2
        n, nbytes = s.shape[0], dw * dh + 2 * cw * ch
        if out is None:
            out = torch.empty((nbytes,) if squeeze else (n, nbytes), dtype=torch.uint8, device=s.device)
        o = out.unsqueeze(0) if out.dim() == 1 else out
        if (o.dtype != torch.uint8 or o.device != s.device or tuple(o.shape) != (n, nbytes) or not o.is_contiguous()):
            raise IqoError("out must be a contiguous uint8 tensor [%d, %d] on %s" % (n, nbytes, s.device))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        wsb = rgb_yuv_workspace_bytes(dw, dh, C, n)
        ws = self._yuv_workspace(wsb, s.device, stream)
        head = (self._plan, n, s.stride(1), s.stride(0), _ptr(s), cs, (ctypes.c_int * 3)(*SOURCE_ORDERS[order]), dw)
        b = o.data_ptr()
        tail = (_ptr(ws), ws.numel(), _stream_ptr(stream))
        if nv12:
            rc = lib().iqo_hip_resize_rgb_nv12_device(*head, 2 * cw, o.stride(0), b, b + dw * dh, *tail)
        else:
            rc = lib().iqo_hip_resize_rgb_yuv420_device(*head, cw, o.stride(0), b, b + dw * dh, b + dw * dh + cw * ch,
                                                        *tail)
        _check(rc, what)
        return out

    def resize_nv12(self, src, standard="bt709", order="rgb", out=None, stream=None):
        """iqo_hip_resize_rgb_nv12_device on torch tensors, for packed resizers with 3 or 4 channels.  src: the
        tensor resize_tensor takes, [F, srcH, srcW, C] (or [srcH, srcW, C]) uint8 on the plan's device; order:
        "rgb" or "bgr", where R, G, B sit in a source pixel (a fourth channel is resized and ignored); standard: a
        COLOR_STANDARDS name or an IQO_CS_* value.  Returns / fills out [F, dstW*dstH + 2*(dstW/2)*(dstH/2)] uint8
        (or one such row), each frame laid out NV12 (Y, then the interleaved UV plane, tightly packed): the
        layout Nv12Resizer.resize_frames takes and gives."""
        return self._resize_yuv(True, src, standard, order, out, stream)

    def resize_i420(self, src, standard="bt709", order="rgb", out=None, stream=None):
        """resize_nv12 with separate chroma planes (iqo_hip_resize_rgb_yuv420_device): each frame laid out I420
        (Y, then U, then V, tightly packed), the layout of Yuv420Resizer.resize_frames."""
        return self._resize_yuv(False, src, standard, order, out, stream)


class LanczosResizer(_Resizer):
    """iqo::LanczosResizer(degree, srcW, srcH, dstW, dstH, pxScale=1) -- LanczosResizer.hpp:26-33.
    channels > 1: interleaved pixels (iqo_hip_plan_packed)."""
    _method = 0

    def __init__(self, degree, srcW, srcH, dstW, dstH, pxScale=1, device=None, channels=1):
        self.degree, self.pxScale = int(degree), int(pxScale)
        super().__init__(srcW, srcH, dstW, dstH, device, channels)

    def _make(self):
        _check(lib().iqo_hip_plan_lanczos(self.degree, self.srcW, self.srcH, self.dstW, self.dstH, self.pxScale,
                                          self.device, ctypes.byref(self._plan)), "LanczosResizer")


class AreaResizer(_Resizer):
    """iqo::AreaResizer(srcW, srcH, dstW, dstH) -- AreaResizer.hpp:24-29."""
    _method = 1

    def _make(self):
        _check(lib().iqo_hip_plan_area(self.srcW, self.srcH, self.dstW, self.dstH, self.device,
                                       ctypes.byref(self._plan)), "AreaResizer")


class LinearResizer(_Resizer):
    """iqo::LinearResizer(srcW, srcH, dstW, dstH) -- LinearResizer.hpp:24-29."""
    _method = 2

    def _make(self):
        _check(lib().iqo_hip_plan_linear(self.srcW, self.srcH, self.dstW, self.dstH, self.device,
                                         ctypes.byref(self._plan)), "LinearResizer")


def make_resizer(method, degree, srcW, srcH, dstW, dstH, pxScale=1, device=None, channels=1):
    if method == "lanczos":
        return LanczosResizer(degree, srcW, srcH, dstW, dstH, pxScale, device, channels)
    if method == "area":
        return AreaResizer(srcW, srcH, dstW, dstH, device, channels)
    if method == "linear":
        return LinearResizer(srcW, srcH, dstW, dstH, device, channels)
    raise ValueError(method)


def _out_code(dtype):
    """(dtype, IQO_OUT_*) of a torch float dtype; None: float32."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    codes = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
    if dtype not in codes:
        raise IqoError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
    return dtype, codes[dtype]


def _roi_out_u8(shape, C, s, out):
    """`out`, or a new tensor on s's device: uint8 [N, dstH, dstW(, C)]."""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=s.device)
    N, dstH, dstW = shape[:3]
    if (out.dtype != torch.uint8 or out.device != s.device or tuple(out.shape) != shape or out.stride(2) != C
            or (out.dim() == 4 and out.stride(3) != 1) or out.stride(1) < dstW * C
            or (N > 1 and out.stride(0) < dstH * out.stride(1))):
        raise IqoError("out must be a uint8 tensor %s on %s with contiguous pixels and non-overlapping rows and "
                       "outputs" % (shape, s.device))
    return out


def _roi_out_norm(shape, dtype, s, out):
    """`out`, or a new tensor on s's device: `dtype` [N, planes, dstH, dstW]."""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=s.device)
    N, planes, dstH, dstW = shape
    if (out.dtype != dtype or out.device != s.device or tuple(out.shape) != shape or out.stride(3) != 1
            or out.stride(2) < dstW or out.stride(1) < dstH * out.stride(2)
            or (N > 1 and out.stride(0) < planes * out.stride(1))):
        raise IqoError("out must be a %s tensor %s on %s with unit column stride and non-overlapping rows, planes "
                       "and outputs" % (dtype, shape, s.device))
    return out


class _RoiPlan:
    """The plan handle of RoiResizer and YuvRoiResizer, released by the entry a class names in _destroy."""

    def __init__(self, method, degree, dstW, dstH, device):
        self.method = _METHODS[method] if isinstance(method, str) else int(method)
        self.degree, self.dstW, self.dstH = int(degree), int(dstW), int(dstH)
        self.device = 0 if device is None else int(device)
        self._plan = _vp()

    def __del__(self):
        p = getattr(self, "_plan", None)
        if p and _lib is not None:
            getattr(_lib, self._destroy)(p)
            self._plan = _vp()


class RoiResizer(_RoiPlan):
    """Crop-and-resize a batch of boxes of device-resident frames to one dstW x dstH in one launch
    (iqo_hip_plan_rois).  method: "lanczos" / "area" / "linear" (or 0 / 1 / 2); channels 1, 3 or 4.  Every output is
    bit for bit the {Lanczos,Area,Linear}Resizer result on the cropped image.  Calls are asynchronous on the stream;
    one call at a time per object (not thread-safe); not capturable into a graph."""

    _destroy = "iqo_hip_roi_plan_destroy"

    def __init__(self, method, degree, dstW, dstH, channels=1, device=None):
        _RoiPlan.__init__(self, method, degree, dstW, dstH, device)
        self.channels = int(channels)
        _check(lib().iqo_hip_plan_rois(self.method, self.degree, self.channels, self.dstW, self.dstH, self.device,
                                       ctypes.byref(self._plan)), "RoiResizer")

    def _source(self, src):
        """src [F, H, W] (channels 1) or [F, H, W, C] uint8 on the device, read where it lies when the pixel bytes
        are contiguous and the row and frame strides are positive (.contiguous() otherwise)."""
        import torch
        C = self.channels
        ok = src.dtype == torch.uint8 and src.is_cuda and (src.dim() == 4 and src.shape[3] == C
                                                           or src.dim() == 3 and C == 1)
        if not ok:
            raise IqoError("expected a uint8 device tensor [F, H, W, %d]%s" % (C, " or [F, H, W]" if C == 1 else ""))
        if src.stride(2) != C or (src.dim() == 4 and src.stride(3) != 1) or min(src.stride(0), src.stride(1)) < 1:
            src = src.contiguous()
        return src

    def resize_rois(self, src, boxes, out=None, stream=None, rects=None, fit=None, pad=0):
        """boxes: a sequence of (frame, x, y, w, h) or (frame, x, y, w, h, flip).  Returns / fills out
        [N, dstH, dstW] (3-dimensional src) or [N, dstH, dstW, C]: a uint8 tensor on src's device with contiguous
        pixels and non-overlapping rows and outputs.
        rects (one (x, y, w, h) of the output per box) or fit ("letterbox", "letterbox-topleft": fit_rects) sends
        each box to a rectangle of its output, resized to the rectangle's size, and fills the rest with `pad` (an
        int, or up to 4 channel bytes), in the same launch (iqo_hip_resize_rois_fit_device)."""
        import torch
        s = self._source(src)
        C, boxes = self.channels, [tuple(b) for b in boxes]
        N = len(boxes)
        out = _roi_out_u8((N, self.dstH, self.dstW) if s.dim() == 3 else (N, self.dstH, self.dstW, C), C, s, out)
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        bad, tail = ctypes.c_int(-1), _fit_args(boxes, self.dstW, self.dstH, rects, fit, pad)
        entry = lib().iqo_hip_resize_rois_fit_device if tail else lib().iqo_hip_resize_rois_device
        rc = entry(self._plan, N, _roi_array(boxes), s.shape[0], s.shape[2], s.shape[1], s.stride(1), s.stride(0), _ptr(s),
                   out.stride(1), out.stride(0), _ptr(out), _stream_ptr(stream), ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "resize_rois")
        return out

    def resize_rois_normalized(self, src, boxes, scale, bias, dtype=None, order=None, out=None, stream=None, rects=None,
                               fit=None, pad=0):
        """As resize_rois, stored as the normalised planar tensor a model takes: [N, planes, dstH, dstW] of `dtype`
        (float32, float16 or bfloat16), plane p = float32(byte of channel order[p]) * scale[p] + bias[p], each
        operation rounded to float32, then rounded to `dtype`.  planes = len(order), or C with the identity order
        (channels 1: order (0, 0, 0) gives grey -> 3 planes).  `out` may be a strided view with unit column stride
        and non-overlapping rows, planes and outputs.  rects / fit / pad as resize_rois: the pad bytes are normalised
        as pixels are."""
        import torch
        dtype, code = _out_code(dtype)
        s = self._source(src)
        boxes = [tuple(b) for b in boxes]
        N = len(boxes)
        n, planes = _norm_of(self.channels, scale, bias, order, code)
        out = _roi_out_norm((N, planes, self.dstH, self.dstW), dtype, s, out)
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        e, bad, tail = out.element_size(), ctypes.c_int(-1), _fit_args(boxes, self.dstW, self.dstH, rects, fit, pad)
        entry = lib().iqo_hip_resize_rois_fit_norm_device if tail else lib().iqo_hip_resize_rois_norm_device
        rc = entry(self._plan, N, _roi_array(boxes), s.shape[0], s.shape[2], s.shape[1], s.stride(1), s.stride(0), _ptr(s),
                   ctypes.byref(n), out.stride(2) * e, out.stride(1) * e, out.stride(0) * e, _ptr(out),
                   _stream_ptr(stream), ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "resize_rois_normalized")
        return out


class YuvRoiResizer(_RoiPlan):
    """Crop-and-resize a batch of boxes of device-resident NV12 / I420 frames to one dstW x dstH, straight to RGB
    bytes or normalised tensors, in one launch (iqo_hip_plan_rois_yuv).  Box coordinates and sizes are even.  Every
    output is bit for bit what Nv12Resizer / Yuv420Resizer(method, degree, w, h, dstW, dstH, chroma="full") gives on
    the cropped frame.  Calls are asynchronous on the stream; one call at a time per object (not thread-safe); not
    capturable into a graph."""

    _destroy = "iqo_hip_roi_yuv_plan_destroy"

    def __init__(self, method, degree, dstW, dstH, layout="nv12", device=None):
        _RoiPlan.__init__(self, method, degree, dstW, dstH, device)
        self.layout = layout
        _check(lib().iqo_hip_plan_rois_yuv(self.method, self.degree, _roi_layout(layout), self.dstW, self.dstH,
                                           self.device, ctypes.byref(self._plan)), "YuvRoiResizer")

    def _source(self, src, frameW, frameH):
        """(nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, Y, U or UV, V) of the tight frame tensor."""
        import torch
        n = frameW * frameH * 3 // 2
        if not (src.dtype == torch.uint8 and src.is_cuda and src.dim() == 2 and src.shape[1] == n):
            raise IqoError("expected a uint8 device tensor [F, %d]" % n)
        if src.stride(1) != 1 or src.stride(0) < 1:
            src = src.contiguous()
        stY, stUV, y, u, v = _yuv_planes(self.layout, src.data_ptr(), frameW, frameH)
        return src, (src.shape[0], frameW, frameH, stY, stUV, src.stride(0), y, u, v)

    def resize_rois_rgb_device(self, boxes, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, dY, dUorUV, dV,
                               dstSt, dstRoiSt, dDst, standard="bt709", order="rgb", stream=None, rects=None, fit=None,
                               pad=0):
        """The raw form (iqo_hip_resize_rois_yuv_rgb_device) for planes that lie anywhere: device addresses (or
        tensors) of frame 0's planes, their row strides and the one frame stride, and the destination's strides, all
        in bytes.  dV is None for NV12.  rects / fit / pad as resize_rois_rgb."""
        boxes = [tuple(b) for b in boxes]
        C, o4 = _rgb_order(order)
        bad, tail = ctypes.c_int(-1), _fit_args(boxes, self.dstW, self.dstH, rects, fit, pad)
        entry = lib().iqo_hip_resize_rois_yuv_fit_rgb_device if tail else lib().iqo_hip_resize_rois_yuv_rgb_device
        rc = entry(
            self._plan, len(boxes), _roi_array(boxes), nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, _ptr(dY),
            _ptr(dUorUV), None if dV is None else _ptr(dV), _standard(standard), C, o4, dstSt, dstRoiSt, _ptr(dDst),
            _stream_ptr(stream), ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "resize_rois_rgb_device")

    def resize_rois_rgb(self, src, boxes, frameW, frameH, standard="bt709", order="rgb", out=None, stream=None,
                        rects=None, fit=None, pad=0):
        """src: uint8 [F, frameW*frameH*3/2] on the device, the tight frames resize_frames of the YUV resizers takes.
        boxes: (frame, x, y, w, h) or (frame, x, y, w, h, flip), all even.  Returns / fills out [N, dstH, dstW, C]
        uint8, C = 3 ("rgb", "bgr") or 4 ("rgba", "bgra"; alpha 255), with contiguous pixels and non-overlapping rows
        and outputs.
        rects (one (x, y, w, h) of the output per box) or fit ("letterbox", "letterbox-topleft": fit_rects) sends
        each box to a rectangle of its output, resized to the rectangle's size, and fills the rest with `pad` (an
        int, or (R, G, B), stored through `order` as a pixel is), in the same launch."""
        import torch
        s, args = self._source(src, frameW, frameH)
        C, _ = _rgb_order(order)
        boxes = [tuple(b) for b in boxes]
        N = len(boxes)
        out = _roi_out_u8((N, self.dstH, self.dstW, C), C, s, out)
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        self.resize_rois_rgb_device(boxes, *args, out.stride(1), out.stride(0), out, standard, order, stream, rects, fit,
                                    pad)
        return out

    def resize_rois_normalized(self, src, boxes, frameW, frameH, scale, bias, standard="bt709", dtype=None,
                               order=(0, 1, 2), out=None, stream=None, rects=None, fit=None, pad=0):
        """As resize_rois_rgb, stored as the normalised planar tensor a model takes: [N, planes, dstH, dstW] of `dtype`
        (float32, float16 or bfloat16), plane p = float32(byte order[p] of (R, G, B)) * scale[p] + bias[p], each
        operation rounded to float32, then rounded to `dtype`.  `out` may be a strided view with unit column stride
        and non-overlapping rows, planes and outputs.  rects / fit / pad as resize_rois_rgb (the letterboxed model
        input in one launch): the pad bytes are normalised as pixels are."""
        import torch
        dtype, code = _out_code(dtype)
        s, args = self._source(src, frameW, frameH)
        boxes = [tuple(b) for b in boxes]
        N = len(boxes)
        n, planes = _norm_of(3, scale, bias, order, code)
        out = _roi_out_norm((N, planes, self.dstH, self.dstW), dtype, s, out)
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        e, bad, tail = out.element_size(), ctypes.c_int(-1), _fit_args(boxes, self.dstW, self.dstH, rects, fit, pad)
        entry = lib().iqo_hip_resize_rois_yuv_fit_norm_device if tail else lib().iqo_hip_resize_rois_yuv_norm_device
        rc = entry(self._plan, N, _roi_array(boxes), *args, _standard(standard), ctypes.byref(n), out.stride(2) * e,
                   out.stride(1) * e, out.stride(0) * e, _ptr(out), _stream_ptr(stream), ctypes.byref(bad), *tail)
        _check_rois(rc, bad, boxes, "resize_rois_normalized")
        return out


class _YuvToRgb:
    """resize_rgb / resize_normalized of the two YUV 4:2:0 resizers: the planes resized as resize_frames
    does, then the integer YUV -> RGB matrix of include/iqo_hip.h (IQO_CS_*) with chroma replicated to the
    output grid, in one more kernel.  With chroma="full" (IQO_CHROMA_FULL) U and V are instead resized
    srcW/2 x srcH/2 -> dstW x dstH (Lanczos: pxScale 1) and every pixel takes its own chroma sample.  The
    subclass supplies _frame_bytes(), _to_rgb() / _to_norm() and the names _SET_CHROMA / _PLANE of its C
    entries."""

    chroma = "replicate"

    def set_chroma(self, chroma):
        """"replicate" or "full" for the later resize_rgb / resize_normalized calls (resize_frames is the same
        in either mode).  The first "full" builds the full-grid chroma plan (plane 2 of set_option); on an
        error (IqoError) the mode stays.  Not while another thread or a captured graph uses the resizer."""
        mode = _chroma(chroma)
        _check(getattr(lib(), self._SET_CHROMA)(self._plan, mode), "%s chroma=%r" % (type(self).__name__, chroma))
        self.chroma = chroma

    def chroma_kernel(self):
        """Kernel name of the full-grid chroma plan, None before the first chroma="full"."""
        p = getattr(lib(), self._PLANE)(self._plan, 2)
        if not p:
            return None
        d = PlanDesc()
        _check(lib().iqo_hip_plan_query(p, ctypes.byref(d)), "query")
        return KERNELS.get(d.kernel, d.kernel)

    def _plane(self, plane):
        p = getattr(lib(), self._PLANE)(self._plan, plane)
        if not p:
            raise IqoError("plane %r: no such sub-plan (plane 2 exists after chroma=\"full\")" % (plane,))
        return p

    def _src_frames(self, src):
        import torch
        n = self._frame_bytes()
        if (src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 2 or src.shape[1] != n
                or not src.is_contiguous()):
            raise IqoError("src must be a contiguous uint8 device tensor [frames, %d]" % n)
        return src

    def _workspace(self, src, stream):
        """The device workspace of a call on `stream`: one per stream, kept on the resizer and grown when a
        batch needs more, so the two passes in flight on a stream never see their block handed to another
        allocation (calls on one stream are ordered; calls on different streams get different blocks).  With
        a raw stream handle the resizer must outlive the work it queued; a torch Stream is also recorded on
        the block, which then outlives the resizer as long as that stream needs it."""
        import torch
        nbytes = yuv_rgb_workspace_bytes(self.dstW, self.dstH, src.shape[0], self.chroma)
        cache = self.__dict__.setdefault("_ws", {})
        key = (src.device, _stream_ptr(stream))
        ws = cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = cache[key] = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
        if hasattr(stream, "cuda_stream"):
            ws.record_stream(stream)
        return ws, ws.numel()

    def resize_rgb(self, src, standard="bt709", order="rgb", out=None, stream=None):
        """src: the tight frame layout of resize_frames.  Returns / fills out [F, dstH, dstW, C] uint8, C = 3
        ("rgb", "bgr") or 4 ("rgba", "bgra"; alpha 255).  standard: a COLOR_STANDARDS name ("bt601", "bt601-full",
        "bt709", "bt709-full") or an IQO_CS_* value.  `out` may be a strided view with interleaved channels and
        non-overlapping rows and frames; it is returned."""
        import torch
        if order not in RGB_ORDERS:
            raise IqoError("order must be one of %s" % ", ".join(sorted(RGB_ORDERS)))
        cs = _standard(standard)
        s = self._src_frames(src)
        o4 = RGB_ORDERS[order]
        C = len(o4)
        shape = (s.shape[0], self.dstH, self.dstW, C)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=s.device)
        o = out
        if (o.dtype != torch.uint8 or o.device != s.device or tuple(o.shape) != shape or o.stride(3) != 1
                or o.stride(2) != C or o.stride(1) < self.dstW * C
                or (o.shape[0] > 1 and o.stride(0) < self.dstH * o.stride(1))):
            raise IqoError("out must be a uint8 tensor [%d, %d, %d, %d] on %s with interleaved channels and "
                           "non-overlapping rows and frames" % (shape + (s.device,)))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        ws, nbytes = self._workspace(s, stream)
        self._to_rgb(s, cs, C, (ctypes.c_int * 4)(*(o4 + (0,) * (4 - C))), o.stride(1), o.stride(0), o, ws, nbytes,
                     stream)
        return out

    def resize_normalized(self, src, scale, bias, standard="bt709", dtype=None, order=(0, 1, 2), out=None,
                          stream=None):
        """src: the tight frame layout of resize_frames.  Returns / fills out [F, planes, dstH, dstW] of `dtype`
        (float32, float16 or bfloat16): plane p is float32(byte order[p] of (R, G, B)) * scale[p] + bias[p], each
        operation rounded to float32, then rounded to `dtype` -- _Resizer.resize_normalized on the RGB bytes of
        resize_rgb.  `out` may be a strided view with unit column stride and non-overlapping rows, planes and
        frames; it is returned."""
        import torch
        if dtype is None:
            dtype = torch.float32
        codes = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
        if dtype not in codes:
            raise IqoError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
        cs = _standard(standard)
        order = tuple(int(c) for c in order)
        scale, bias = tuple(float(v) for v in scale), tuple(float(v) for v in bias)
        planes = len(order)
        if not 1 <= planes <= 4 or len(scale) != planes or len(bias) != planes:
            raise IqoError("order, scale and bias must have the same length, 1..4 (one entry per output plane)")
        s = self._src_frames(src)
        shape = (s.shape[0], planes, self.dstH, self.dstW)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=s.device)
        o = out
        if (o.dtype != dtype or o.device != s.device or tuple(o.shape) != shape or o.stride(3) != 1
                or o.stride(2) < self.dstW or o.stride(1) < self.dstH * o.stride(2)
                or (o.shape[0] > 1 and o.stride(0) < planes * o.stride(1))):
            raise IqoError("out must be a %s tensor [%d, %d, %d, %d] on %s with unit column stride and "
                           "non-overlapping rows, planes and frames" % ((dtype,) + shape + (s.device,)))
        if stream is None:
            stream = torch.cuda.current_stream(s.device)
        n = Norm(codes[dtype], planes)
        for i in range(planes):
            n.order[i], n.scale[i], n.bias[i] = order[i], scale[i], bias[i]
        e = o.element_size()
        ws, nbytes = self._workspace(s, stream)
        self._to_norm(s, cs, n, o.stride(2) * e, o.stride(1) * e, o.stride(0) * e, o, ws, nbytes, stream)
        return out


    def resize_luma_normalized(self, src, scale, bias, dtype=None, out=None, stream=None):
        """Luma only, for models that take no colour: the Y plane of each frame resized by plane 0's plan and
        written as `planes` = len(scale) = len(bias) (1..4) normalised planes, all taken from Y
        (iqo_hip_resize_planes_norm_device with srcPlanes 1 and order all zero).  src: the tight frame layout of
        resize_frames.  Chroma is neither resized nor read, and the chroma mode has no effect.  Returns / fills
        out [F, planes, dstH, dstW] of `dtype` as resize_normalized does."""
        s = self._src_frames(src)
        scale = tuple(scale)
        layout = (s.shape[0], 1, self.srcW, 0, s.stride(0), s.data_ptr())
        return _planes_norm(self, "resize_luma_normalized", self._plane(0), s, layout, scale, bias, dtype,
                            (0,) * len(scale), False, out, stream)


class Yuv420Resizer(_YuvToRgb):
    """I420 three-plane resizer: the reference benchmark's workload (benchmark.cpp:131-229), Y at
    full size and U, V at half size with the same method (Lanczos chroma: pxScale 2).  chroma: "replicate" or
    "full", how resize_rgb / resize_normalized bring chroma to the output grid (_YuvToRgb)."""

    _SET_CHROMA, _PLANE = "iqo_hip_yuv_plan_set_chroma", "iqo_hip_yuv_plane"

    def __init__(self, method, degree, srcW, srcH, dstW, dstH, device=None, chroma="replicate"):
        mode = _chroma(chroma)
        self.method, self.degree = method, int(degree)
        self.srcW, self.srcH, self.dstW, self.dstH = int(srcW), int(srcH), int(dstW), int(dstH)
        self.device = 0 if device is None else int(device)
        self._plan = _vp()
        _check(lib().iqo_hip_plan_yuv420(_METHODS[method], self.degree, self.srcW, self.srcH, self.dstW, self.dstH,
                                         self.device, ctypes.byref(self._plan)), "Yuv420Resizer")
        if mode != CHROMA_REPLICATE:
            self.set_chroma(chroma)

    def __del__(self):
        p = getattr(self, "_plan", None)
        if p and _lib is not None:
            _lib.iqo_hip_yuv_plan_destroy(p)
            self._plan = _vp()

    def set_option(self, key, value, plane=None):
        """plane: 0 luma, 1 chroma, 2 the full-grid chroma plan of chroma="full"; None: planes 0 and 1."""
        for pl in ((0, 1) if plane is None else (plane,)):
            _check(lib().iqo_hip_plan_set_option(self._plane(pl), key.encode(), int(value)), "set_option")

    def resize(self, srcStY, srcY, srcStUV, srcU, srcV, dstStY, dstY, dstStUV, dstU, dstV):
        """Host pointers, synchronous."""
        _check(lib().iqo_hip_resize_yuv420(self._plan, srcStY, _ptr(srcY), srcStUV, _ptr(srcU), _ptr(srcV), dstStY,
                                           _ptr(dstY), dstStUV, _ptr(dstU), _ptr(dstV)), "resize_yuv420")

    def resize_device(self, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcU, srcV, dstStY, dstStUV, dstFrameSt,
                      dstY, dstU, dstV, stream=None):
        """Device-resident batch (async on `stream`); returns True when one launch did all planes."""
        fused = ctypes.c_int(0)
        _check(lib().iqo_hip_resize_yuv420_device(self._plan, nFrames, srcStY, srcStUV, srcFrameSt, _ptr(srcY),
                                                  _ptr(srcU), _ptr(srcV), dstStY, dstStUV, dstFrameSt, _ptr(dstY),
                                                  _ptr(dstU), _ptr(dstV), _stream_ptr(stream), ctypes.byref(fused)),
               "resize_yuv420_device")
        return bool(fused.value)

    def resize_frames(self, src, out=None, stream=None):
        """src: uint8 CUDA tensor [frames, srcH*3/2 * srcW] per frame laid out I420 (Y, then U, then V,
        tightly packed); returns / fills out [frames, dstH*3/2 * dstW].  Returns (out, fused)."""
        import torch
        sw, sh, dw, dh = self.srcW, self.srcH, self.dstW, self.dstH
        cs, cd = (sw // 2) * (sh // 2), (dw // 2) * (dh // 2)
        if (src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 2 or src.shape[1] != sw * sh + 2 * cs
                or not src.is_contiguous()):
            raise IqoError("src must be a contiguous uint8 device tensor [frames, %d]" % (sw * sh + 2 * cs))
        n = src.shape[0]
        if out is None:
            out = torch.empty((n, dw * dh + 2 * cd), dtype=torch.uint8, device=src.device)
        if (out.dtype != torch.uint8 or out.device != src.device or tuple(out.shape) != (n, dw * dh + 2 * cd)
                or not out.is_contiguous()):
            raise IqoError("out must be a contiguous uint8 tensor [%d, %d] on %s" % (n, dw * dh + 2 * cd, src.device))
        b, o = src.data_ptr(), out.data_ptr()
        fused = self.resize_device(n, sw, sw // 2, src.stride(0), b, b + sw * sh, b + sw * sh + cs,
                                   dw, dw // 2, out.stride(0), o, o + dw * dh, o + dw * dh + cd, stream)
        return out, fused

    # -- _YuvToRgb: the I420 entries; last_fused tells whether the first pass of the last call was one launch
    last_fused = False

    def _frame_bytes(self):
        return self.srcW * self.srcH + 2 * (self.srcW // 2) * (self.srcH // 2)

    def _src_args(self, s):
        sw, sh = self.srcW, self.srcH
        b, cs = s.data_ptr(), (sw // 2) * (sh // 2)
        return (self._plan, s.shape[0], sw, sw // 2, s.stride(0), b, b + sw * sh, b + sw * sh + cs)

    def _to_rgb(self, s, cs, C, order, row_st, frame_st, o, ws, nbytes, stream):
        fused = ctypes.c_int(0)
        _check(lib().iqo_hip_resize_yuv420_rgb_device(*self._src_args(s), cs, C, order, row_st, frame_st, _ptr(o),
                                                      _ptr(ws), nbytes, _stream_ptr(stream), ctypes.byref(fused)),
               "resize_rgb")
        self.last_fused = bool(fused.value)

    def _to_norm(self, s, cs, norm, row_st, plane_st, frame_st, o, ws, nbytes, stream):
        fused = ctypes.c_int(0)
        _check(lib().iqo_hip_resize_yuv420_norm_device(*self._src_args(s), cs, ctypes.byref(norm), row_st, plane_st,
                                                       frame_st, _ptr(o), _ptr(ws), nbytes, _stream_ptr(stream),
                                                       ctypes.byref(fused)), "resize_normalized")
        self.last_fused = bool(fused.value)


class Nv12Resizer(_YuvToRgb):
    """NV12 resizer: a planar Y plane at full size and one interleaved UV plane at half size, with
    the same method (Lanczos chroma: pxScale 2).  U and V come out as Yuv420Resizer's planes do.  chroma:
    "replicate" or "full", how resize_rgb / resize_normalized bring chroma to the output grid (_YuvToRgb)."""

    _SET_CHROMA, _PLANE = "iqo_hip_nv12_plan_set_chroma", "iqo_hip_nv12_plane"

    def __init__(self, method, degree, srcW, srcH, dstW, dstH, device=None, chroma="replicate"):
        mode = _chroma(chroma)
        self.method, self.degree = method, int(degree)
        self.srcW, self.srcH, self.dstW, self.dstH = int(srcW), int(srcH), int(dstW), int(dstH)
        self.device = 0 if device is None else int(device)
        self._plan = _vp()
        _check(lib().iqo_hip_plan_nv12(_METHODS[method], self.degree, self.srcW, self.srcH, self.dstW, self.dstH,
                                       self.device, ctypes.byref(self._plan)), "Nv12Resizer")
        if mode != CHROMA_REPLICATE:
            self.set_chroma(chroma)

    def __del__(self):
        p = getattr(self, "_plan", None)
        if p and _lib is not None:
            _lib.iqo_hip_nv12_plan_destroy(p)
            self._plan = _vp()

    def set_option(self, key, value, plane=None):
        """plane: 0 luma, 1 UV, 2 the full-grid UV plan of chroma="full"; None: planes 0 and 1."""
        for pl in ((0, 1) if plane is None else (plane,)):
            _check(lib().iqo_hip_plan_set_option(self._plane(pl), key.encode(), int(value)), "set_option")

    def describe(self):
        """Kernel names of the (Y, UV) plans."""
        out = []
        for pl in (0, 1):
            d = PlanDesc()
            _check(lib().iqo_hip_plan_query(lib().iqo_hip_nv12_plane(self._plan, pl), ctypes.byref(d)), "query")
            out.append(KERNELS.get(d.kernel, d.kernel))
        return tuple(out)

    def resize_device(self, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcUV, dstStY, dstStUV, dstFrameSt, dstY,
                      dstUV, stream=None):
        """Device-resident batch (async on `stream`); strides in bytes."""
        _check(lib().iqo_hip_resize_nv12_device(self._plan, nFrames, srcStY, srcStUV, srcFrameSt, _ptr(srcY),
                                                _ptr(srcUV), dstStY, dstStUV, dstFrameSt, _ptr(dstY), _ptr(dstUV),
                                                _stream_ptr(stream)), "resize_nv12_device")

    def resize_frames(self, src, out=None, stream=None):
        """src: uint8 CUDA tensor [frames, srcH*srcW + 2*(srcW/2)*(srcH/2)], each frame laid out NV12 (Y, then
        the interleaved UV plane, tightly packed); returns / fills out in the same layout at the output size."""
        import torch
        sw, sh, dw, dh = self.srcW, self.srcH, self.dstW, self.dstH
        cs, cd = 2 * (sw // 2) * (sh // 2), 2 * (dw // 2) * (dh // 2)
        if (src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 2 or src.shape[1] != sw * sh + cs
                or not src.is_contiguous()):
            raise IqoError("src must be a contiguous uint8 device tensor [frames, %d]" % (sw * sh + cs))
        n = src.shape[0]
        if out is None:
            out = torch.empty((n, dw * dh + cd), dtype=torch.uint8, device=src.device)
        if (out.dtype != torch.uint8 or out.device != src.device or tuple(out.shape) != (n, dw * dh + cd)
                or not out.is_contiguous()):
            raise IqoError("out must be a contiguous uint8 tensor [%d, %d] on %s" % (n, dw * dh + cd, src.device))
        if stream is None:
            stream = torch.cuda.current_stream(src.device)
        b, o = src.data_ptr(), out.data_ptr()
        self.resize_device(n, sw, 2 * (sw // 2), src.stride(0), b, b + sw * sh, dw, 2 * (dw // 2), out.stride(0),
                           o, o + dw * dh, stream)
        return out

    # -- _YuvToRgb: the NV12 entries
    def _frame_bytes(self):
        return self.srcW * self.srcH + 2 * (self.srcW // 2) * (self.srcH // 2)

    def _src_args(self, s):
        sw, sh = self.srcW, self.srcH
        b = s.data_ptr()
        return (self._plan, s.shape[0], sw, 2 * (sw // 2), s.stride(0), b, b + sw * sh)

    def _to_rgb(self, s, cs, C, order, row_st, frame_st, o, ws, nbytes, stream):
        _check(lib().iqo_hip_resize_nv12_rgb_device(*self._src_args(s), cs, C, order, row_st, frame_st, _ptr(o),
                                                    _ptr(ws), nbytes, _stream_ptr(stream)), "resize_rgb")

    def _to_norm(self, s, cs, norm, row_st, plane_st, frame_st, o, ws, nbytes, stream):
        _check(lib().iqo_hip_resize_nv12_norm_device(*self._src_args(s), cs, ctypes.byref(norm), row_st, plane_st,
                                                     frame_st, _ptr(o), _ptr(ws), nbytes, _stream_ptr(stream)),
               "resize_normalized")
