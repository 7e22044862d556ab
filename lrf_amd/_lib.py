"""ctypes binding of liblrf_hip.so (include/lrf_hip.h).  There is no CPU fallback: if the HIP
library is missing or no GPU is visible, the calls raise."""
import ctypes
import functools
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblrf_hip.so")

LRF_MAX_RANK = 64
LRF_K_PLANES, LRF_K_INIT, LRF_K_BCD, LRF_K_VUPDATE, LRF_K_DECODE, LRF_K_GRAM, LRF_K_BCD_PERSIST, LRF_K_PLANES_GRAM, LRF_K_METRICS = range(9)
LRF_DEFLATE_CG = 8  # columns per workgroup of lrf_deflate_sizes_i8 (include/lrf_hip.h)
LRF_K_INFLATE = 9  # behind LRF_K_COUNT (include/lrf_hip.h): timed like the others, no step of bench.py's sequences (not in KERNEL_NAMES)
KERNEL_NAMES = {LRF_K_PLANES: "k_planes", LRF_K_GRAM: "k_gram", LRF_K_INIT: "k_init", LRF_K_BCD: "k_bcd",
                LRF_K_VUPDATE: "k_vupdate", LRF_K_DECODE: "k_decode", LRF_K_BCD_PERSIST: "k_bcd_persist",
                LRF_K_PLANES_GRAM: "k_planes_gram", LRF_K_METRICS: "k_metrics"}

_lib = None
_lock = threading.Lock()

c_void_p, c_int, c_i64, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t


class LrfError(RuntimeError):
    pass


class QmfOpts(ctypes.Structure):
    """lrf_qmf_opts (include/lrf_hip.h)"""
    _fields_ = [("bounded", c_int), ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("l2_u", ctypes.c_double), ("l2_v", ctypes.c_double),
                ("l1_ratio", ctypes.c_double), ("factors", c_int), ("eps", ctypes.c_double), ("w_init", c_int)]


class RaggedImage(ctypes.Structure):
    """lrf_ragged_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("R", c_int * 3), ("u_off", c_i64), ("v_off", c_i64), ("rgb_off", c_i64)]


class Crop(ctypes.Structure):
    """lrf_crop (include/lrf_hip.h)"""
    _fields_ = [("image", ctypes.c_int32), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32)]


class ScaledCrop(ctypes.Structure):
    """lrf_scaled_crop (include/lrf_hip.h)"""
    _fields_ = [("image", ctypes.c_int32), ("scale", ctypes.c_int32), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32)]


class ResizedCrop(ctypes.Structure):
    """lrf_resized_crop (include/lrf_hip.h)"""
    _fields_ = [("image", ctypes.c_int32), ("y0", ctypes.c_int32), ("x0", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("flip", ctypes.c_int32)]


class TensorFormat(ctypes.Structure):
    """lrf_tensor_format (include/lrf_hip.h)"""
    _fields_ = [("dtype", ctypes.c_int32), ("layout", ctypes.c_int32), ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3)]


class GrayImage(ctypes.Structure):
    """lrf_gray_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("R", c_int), ("u_off", c_i64), ("v_off", c_i64), ("out_off", c_i64)]


class RaggedEncodeImage(ctypes.Structure):
    """lrf_ragged_encode_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("R", c_int * 3), ("rgb_off", c_i64), ("u_off", c_i64), ("v_off", c_i64), ("sign_off", c_i64)]


class RaggedSweepImage(ctypes.Structure):
    """lrf_ragged_sweep_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("rgb_off", c_i64), ("sign_off", c_i64)]


class RaggedSweepCandidate(ctypes.Structure):
    """lrf_ragged_sweep_candidate (include/lrf_hip.h)"""
    _fields_ = [("image", ctypes.c_int32), ("R", c_int * 3), ("u_off", c_i64), ("v_off", c_i64)]


class GraySweepImage(ctypes.Structure):
    """lrf_gray_sweep_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("gray_off", c_i64), ("sign_off", c_i64)]


class GraySweepCandidate(ctypes.Structure):
    """lrf_gray_sweep_candidate (include/lrf_hip.h)"""
    _fields_ = [("image", ctypes.c_int32), ("R", c_int), ("u_off", c_i64), ("v_off", c_i64)]


class GrayEncodeImage(ctypes.Structure):
    """lrf_gray_encode_image (include/lrf_hip.h)"""
    _fields_ = [("H", c_i64), ("W", c_i64), ("R", c_int), ("gray_off", c_i64), ("u_off", c_i64), ("v_off", c_i64), ("sign_off", c_i64)]


def load():
    """Loads liblrf_hip.so; raises ImportError when it has not been built (see __graft_entry__.build)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build the HIP extension first "
                              "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        lib.lrf_last_error.restype = ctypes.c_char_p
        lib.lrf_ctx_workspace_bytes.restype = c_size_t
        lib.lrf_ctx_workspace_bytes.argtypes = [c_void_p]
        lib.lrf_ctx_create.argtypes = [c_int, ctypes.POINTER(c_void_p)]
        lib.lrf_ctx_destroy.argtypes = [c_void_p]
        lib.lrf_ctx_destroy.restype = None
        lib.lrf_ctx_set_stream.argtypes = [c_void_p, c_void_p]
        lib.lrf_ctx_use_own_stream.argtypes = [c_void_p]
        lib.lrf_ctx_synchronize.argtypes = [c_void_p]
        lib.lrf_ctx_check.argtypes = [c_void_p]
        lib.lrf_ctx_last_luma_source.argtypes = [c_void_p]
        lib.lrf_ctx_last_x_residency.argtypes = [c_void_p, ctypes.POINTER(c_i64)]
        lib.lrf_ctx_trim.argtypes = [c_void_p]
        lib.lrf_ctx_profile.argtypes = [c_void_p, c_int]
        lib.lrf_ctx_profile_reset.argtypes = [c_void_p]
        lib.lrf_ctx_profile_kernels.argtypes = [c_void_p, ctypes.c_uint]
        lib.lrf_ctx_kernel_time.argtypes = [c_void_p, c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        lib.lrf_malloc.argtypes = [c_void_p, c_size_t, ctypes.POINTER(c_void_p)]
        lib.lrf_free.argtypes = [c_void_p, c_void_p]
        lib.lrf_memcpy_h2d.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
        lib.lrf_memcpy_d2h.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
        lib.lrf_plane_dims.argtypes = [c_i64, c_i64, c_int] + [ctypes.POINTER(c_i64)] * 5
        lib.lrf_qmf_planes_from_rgb_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p]
        lib.lrf_qmf_decompose_f32.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int,
                                              c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_bcd_f32.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_decompose_ex_f32.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, ctypes.POINTER(QmfOpts), c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_svd_init_f32.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_loss_f32.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p]
        lib.lrf_qmf_encode_rgb_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, ctypes.POINTER(c_int), c_int, c_int,
                                              c_int, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_encode_sweep_rgb_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, ctypes.POINTER(c_int), c_int, c_int,
                                                    c_int, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_decode_rgb_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, ctypes.POINTER(c_int),
                                              c_void_p]
        lib.lrf_qmf_decode_ragged_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_crops_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64, ctypes.POINTER(Crop),
                                                    c_i64, c_i64, c_void_p, c_i64]
        lib.lrf_scaled_dims.argtypes = [c_i64, c_i64, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]
        lib.lrf_qmf_decode_scaled_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_scaled_crops_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64,
                                                           ctypes.POINTER(ScaledCrop), c_i64, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_resized_crops_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64,
                                                            ctypes.POINTER(ResizedCrop), c_i64, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_crops_tensor.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64, ctypes.POINTER(Crop),
                                                    c_i64, c_i64, ctypes.POINTER(TensorFormat), c_void_p, c_i64]
        lib.lrf_qmf_decode_scaled_crops_tensor.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64,
                                                           ctypes.POINTER(ScaledCrop), c_i64, c_i64, ctypes.POINTER(TensorFormat), c_void_p, c_i64]
        lib.lrf_qmf_decode_resized_crops_tensor.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_i64,
                                                            ctypes.POINTER(ResizedCrop), c_i64, c_i64, ctypes.POINTER(TensorFormat), c_void_p, c_i64]
        lib.lrf_qmf_encode_ragged_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedEncodeImage), c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_i64,
                                                     c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_encode_ragged_sweep_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedSweepImage), c_i64, ctypes.POINTER(RaggedSweepCandidate),
                                                           c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_sse_ragged_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]
        lib.lrf_image_metrics_ragged_u8.argtypes = [c_void_p, c_i64, c_void_p, c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p]
        lib.lrf_qmf_ssim_ragged_rgb_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(RaggedImage), c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_i64,
                                                   c_void_p, c_void_p]
        lib.lrf_deflate_bound.restype = c_i64
        lib.lrf_deflate_bound.argtypes = [c_i64]
        lib.lrf_deflate_columns_i8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_deflate_sizes_i8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_i64]
        lib.lrf_inflate_columns_i8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p]
        lib.lrf_image_metrics_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
        lib.lrf_qmf_sweep_sse_rgb_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, ctypes.POINTER(c_int), c_void_p]
        lib.lrf_svd_encode_rgb_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.lrf_svd_decode_rgb_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p, c_void_p]
        lib.lrf_qmf_rgbspace_encode_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p]
        lib.lrf_qmf_rgbspace_decode_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p]
        lib.lrf_quantize_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p]
        lib.lrf_svd_decode_any_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]
        lib.lrf_rgbspace_dims_any.argtypes = [c_i64, c_i64, c_int, c_int] + [ctypes.POINTER(c_i64)] * 4
        lib.lrf_qmf_rgbspace_matrix_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_void_p]
        lib.lrf_qmf_rgbspace_decode_any_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p]
        lib.lrf_chan_dims.argtypes = [c_i64, c_i64, c_i64, c_int, c_int] + [ctypes.POINTER(c_i64)] * 4
        lib.lrf_qmf_encode_gray_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p]
        lib.lrf_qmf_decode_gray_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_void_p]
        gray_list = [c_void_p, c_i64, ctypes.POINTER(GrayImage), c_void_p, c_i64, c_void_p, c_i64, c_i64]
        lib.lrf_qmf_decode_gray_ragged_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(GrayImage), c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_gray_crops_u8.argtypes = gray_list + [ctypes.POINTER(ScaledCrop), c_i64, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_gray_crops_tensor.argtypes = gray_list + [ctypes.POINTER(ScaledCrop), c_i64, c_i64, ctypes.POINTER(TensorFormat), c_void_p, c_i64]
        lib.lrf_qmf_decode_gray_resized_crops_u8.argtypes = gray_list + [ctypes.POINTER(ResizedCrop), c_i64, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_decode_gray_resized_crops_tensor.argtypes = gray_list + [ctypes.POINTER(ResizedCrop), c_i64, c_i64, ctypes.POINTER(TensorFormat), c_void_p,
                                                                             c_i64]
        lib.lrf_qmf_encode_gray_ragged_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(GrayEncodeImage), c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_i64,
                                                      c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_encode_gray_ragged_sweep_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(GraySweepImage), c_i64, ctypes.POINTER(GraySweepCandidate),
                                                            c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64]
        lib.lrf_qmf_sse_gray_ragged_u8.argtypes = [c_void_p, c_i64, ctypes.POINTER(GrayImage), c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]
        lib.lrf_qmf_chan_matrix_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_void_p]
        lib.lrf_qmf_chan_decode_u8.argtypes = [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p]
        lib.lrf_plane_dims_any.argtypes = [c_i64, c_i64, c_int, c_int, c_int] + [ctypes.POINTER(c_i64)] * 6
        lib.lrf_plane_dims_any_hw.argtypes = [c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int] + [ctypes.POINTER(c_i64)] * 6
        lib.lrf_qmf_planes_any_hw_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p]
        lib.lrf_qmf_decode_any_hw_u8.argtypes = [c_void_p] + [c_void_p] * 6 + [c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int,
                                                                              ctypes.POINTER(c_int), c_void_p]
        lib.lrf_qmf_planes_any_u8.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p]
        lib.lrf_qmf_decode_any_u8.argtypes = [c_void_p] + [c_void_p] * 6 + [c_i64, c_i64, c_i64, c_int, c_int,
                                                                           ctypes.POINTER(c_int), c_void_p]
        lib.lrf_pipe_create.argtypes = [c_int, c_int, c_i64, ctypes.POINTER(c_void_p)]
        lib.lrf_pipe_destroy.argtypes = [c_void_p]
        lib.lrf_pipe_destroy.restype = None
        lib.lrf_pipe_slots.argtypes = [c_void_p]
        lib.lrf_pipe_slot_ctx.argtypes = [c_void_p, c_int]
        lib.lrf_pipe_slot_ctx.restype = c_void_p
        lib.lrf_pipe_workspace_bytes.argtypes = [c_void_p]
        lib.lrf_pipe_workspace_bytes.restype = c_size_t
        lib.lrf_pipe_qmf_encode_rgb_u8_host.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, ctypes.POINTER(c_int), c_int,
                                                        c_int, c_int, c_void_p, c_void_p, c_void_p]
        lib.lrf_pipe_qmf_encode_submit.argtypes = [c_void_p, c_void_p, c_i64, c_i64, c_i64, ctypes.POINTER(c_int), c_int, c_int,
                                                   c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int)]
        lib.lrf_pipe_wait_next.argtypes = [c_void_p, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]
        lib.lrf_host_alloc.argtypes = [c_size_t, ctypes.POINTER(c_void_p)]
        lib.lrf_host_free.argtypes = [c_void_p]
        lib.lrf_host_register.argtypes = [c_void_p, c_size_t]
        lib.lrf_host_unregister.argtypes = [c_void_p]
        _lib = lib
        return lib


EXPORTS = ["lrf_last_error", "lrf_device_count", "lrf_version", "lrf_ctx_create", "lrf_ctx_destroy", "lrf_ctx_set_stream", "lrf_ctx_use_own_stream",
           "lrf_ctx_synchronize", "lrf_ctx_check", "lrf_ctx_last_luma_source", "lrf_ctx_last_x_residency", "lrf_ctx_workspace_bytes", "lrf_ctx_trim", "lrf_ctx_profile", "lrf_ctx_profile_kernels", "lrf_ctx_kernel_time",
           "lrf_ctx_profile_reset", "lrf_malloc", "lrf_free", "lrf_memcpy_h2d", "lrf_memcpy_d2h", "lrf_plane_dims",
           "lrf_qmf_planes_from_rgb_u8", "lrf_qmf_decompose_f32", "lrf_qmf_decompose_ex_f32", "lrf_qmf_bcd_f32", "lrf_qmf_svd_init_f32", "lrf_qmf_loss_f32",
           "lrf_qmf_encode_rgb_u8", "lrf_qmf_encode_sweep_rgb_u8", "lrf_qmf_decode_rgb_u8", "lrf_qmf_decode_ragged_rgb_u8", "lrf_qmf_decode_crops_rgb_u8", "lrf_scaled_dims", "lrf_qmf_decode_scaled_rgb_u8", "lrf_qmf_decode_scaled_crops_rgb_u8", "lrf_qmf_decode_resized_crops_rgb_u8", "lrf_qmf_decode_crops_tensor", "lrf_qmf_decode_scaled_crops_tensor", "lrf_qmf_decode_resized_crops_tensor", "lrf_qmf_encode_ragged_rgb_u8", "lrf_qmf_encode_ragged_sweep_rgb_u8", "lrf_qmf_sse_ragged_rgb_u8", "lrf_image_metrics_ragged_u8", "lrf_qmf_ssim_ragged_rgb_u8", "lrf_deflate_bound", "lrf_deflate_columns_i8", "lrf_deflate_sizes_i8", "lrf_inflate_columns_i8", "lrf_image_metrics_u8", "lrf_qmf_sweep_sse_rgb_u8", "lrf_svd_encode_rgb_u8", "lrf_svd_decode_rgb_u8",
           "lrf_qmf_rgbspace_encode_u8", "lrf_qmf_rgbspace_decode_u8", "lrf_rgbspace_dims_any", "lrf_qmf_rgbspace_matrix_u8",
           "lrf_qmf_rgbspace_decode_any_u8", "lrf_quantize_u8", "lrf_svd_decode_any_u8",
           "lrf_chan_dims", "lrf_qmf_encode_gray_u8", "lrf_qmf_decode_gray_u8", "lrf_qmf_decode_gray_ragged_u8", "lrf_qmf_decode_gray_crops_u8",
           "lrf_qmf_decode_gray_crops_tensor", "lrf_qmf_decode_gray_resized_crops_u8", "lrf_qmf_decode_gray_resized_crops_tensor",
           "lrf_qmf_encode_gray_ragged_u8", "lrf_qmf_encode_gray_ragged_sweep_u8", "lrf_qmf_sse_gray_ragged_u8", "lrf_qmf_chan_matrix_u8", "lrf_qmf_chan_decode_u8",
           "lrf_plane_dims_any", "lrf_qmf_planes_any_u8", "lrf_qmf_decode_any_u8", "lrf_plane_dims_any_hw", "lrf_qmf_planes_any_hw_u8",
           "lrf_qmf_decode_any_hw_u8",
           "lrf_pipe_create", "lrf_pipe_destroy", "lrf_pipe_slots", "lrf_pipe_slot_ctx", "lrf_pipe_workspace_bytes",
           "lrf_pipe_qmf_encode_rgb_u8_host", "lrf_pipe_qmf_encode_submit", "lrf_pipe_wait_next",
           "lrf_host_alloc", "lrf_host_free", "lrf_host_register", "lrf_host_unregister"]


def check(rc):
    if rc == 0:
        return
    msg = load().lrf_last_error().decode(errors="replace")
    if rc == -1:
        raise ValueError(msg)
    if rc == -2:
        raise NotImplementedError(msg)
    if rc == -4:
        raise MemoryError(msg)
    raise LrfError(msg)


@functools.lru_cache(maxsize=8192)
def _plane_dims_of(H, W):
    out = []
    for c in range(3):
        v = [c_i64() for _ in range(5)]
        check(load().lrf_plane_dims(H, W, c, *[ctypes.byref(x) for x in v]))
        out.append(tuple(int(x.value) for x in v))
    return tuple(out)


def plane_dims(H, W):
    """[(h, w, hp, wp, M)] of the Y, Cb, Cr planes of an H x W image (host-only arithmetic; remembered per size: lists of many
    images ask for few distinct sizes)."""
    return list(_plane_dims_of(int(H), int(W)))


def plane_patches(H, W):
    """int64 array [n, 3]: the patch counts M of the Y, Cb, Cr planes for arrays H, W of n sizes, plane_dims asked once per distinct size"""
    H, W = np.asarray(H, dtype=np.int64).reshape(-1), np.asarray(W, dtype=np.int64).reshape(-1)
    sizes, inverse = np.unique(np.stack([H, W], axis=1), axis=0, return_inverse=True)
    Ms = np.array([[d[4] for d in plane_dims(int(h), int(w))] for h, w in sizes], dtype=np.int64).reshape(-1, 3)
    return Ms[inverse.reshape(-1)]


# the C structures as numpy records (same layout: checked against ctypes.sizeof where they are used)
_RAGGED_IMAGE_DT = np.dtype([("H", "<i8"), ("W", "<i8"), ("R", "<i4", (3,)), ("u_off", "<i8"), ("v_off", "<i8"), ("rgb_off", "<i8")], align=True)
_SWEEP_CAND_DT = np.dtype([("image", "<i4"), ("R", "<i4", (3,)), ("u_off", "<i8"), ("v_off", "<i8")], align=True)


def plane_dims_any(H, W, patch_size, chroma=None):
    """[(h, w, hp, wp, M, N)] of the Y, Cb, Cr planes for patches (p, q); patch_size None = patch=False (M, N = h, w).
    chroma: (hc, wc) for a scale_factor other than (0.5, 0.5); None = floor(H / 2) x floor(W / 2)."""
    p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
    hc, wc = (0, 0) if chroma is None else (int(chroma[0]), int(chroma[1]))
    out = []
    for c in range(3):
        v = [c_i64() for _ in range(6)]
        check(load().lrf_plane_dims_any_hw(H, W, hc, wc, p, q, c, *[ctypes.byref(x) for x in v]))
        out.append(tuple(int(x.value) for x in v))
    return out


def chroma_size(H, W, scale_factor):
    """floor(H * s_h) x floor(W * s_w): what F.interpolate(scale_factor=...) produces (lrf/compression/utils.py:92-94); None for
    the default (0.5, 0.5)"""
    import math
    if tuple(scale_factor) == (0.5, 0.5):
        return None
    return (int(math.floor(float(H) * float(scale_factor[0]))), int(math.floor(float(W) * float(scale_factor[1]))))


def rgbspace_dims_any(H, W, patch_size):
    """(Hp, Wp, M, N) of the RGB colour-space branch for patches (p, q); patch_size None = patch=False (per channel [H, W])."""
    p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
    v = [c_i64() for _ in range(4)]
    check(load().lrf_rgbspace_dims_any(H, W, p, q, *[ctypes.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def chan_dims(H, W, C, patch_size):
    """(Hp, Wp, M, N) of a [C,H,W] image in the RGB colour-space branch (lrf_chan_dims: host-only arithmetic): patches (p, q)
    give one matrix [M, C p q]; patch_size None = patch=False, per channel the plane [H, W]"""
    p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
    v = [c_i64() for _ in range(4)]
    check(load().lrf_chan_dims(int(H), int(W), int(C), p, q, *[ctypes.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def chan_rank(M, N, rank=None, quality=None):
    """the scalar rank of the RGB colour-space branch: R = max(round(min(M, N) * quality / 100), 1) (qmf.py:172-178, 196-202)"""
    if rank is not None:
        return int(rank)
    assert quality >= 0 and quality <= 100, "'quality' must be between 0 and 100."
    return max(round(min(M, N) * quality / 100), 1)


def chan_stream_geometry(metadata, u_shape, v_shape):
    """The header walk of a two-factor RGB colour-space stream, host only: -> (C, H, W, patch_size or None, R).  With patches
    C = v.shape[0] / (p q), which must divide, and u, v and the padded size must be the geometry's; with patch=False C is
    u.shape[0] and the image size the factors'.  ValueError for anything else: the kernels index the factors from these numbers."""
    R = int(metadata["rank"])
    if R < 1:
        raise ValueError("stream metadata: 'rank' must be a positive integer")
    u_shape, v_shape = tuple(int(x) for x in u_shape), tuple(int(x) for x in v_shape)
    if metadata["patch"]:
        p, q = (int(x) for x in metadata["patch size"])
        H, W = (int(x) for x in metadata["original size"])
        if p < 1 or q < 1 or len(u_shape) != 2 or len(v_shape) != 2:
            raise ValueError("stream factors are not [M, R] / [C p q, R]")
        if v_shape[0] % (p * q) or v_shape[0] == 0:
            raise ValueError(f"stream factor v has {v_shape[0]} rows: not a multiple of the {p}x{q} patch")
        C = v_shape[0] // (p * q)
        Hp, Wp, M, N = chan_dims(H, W, C, (p, q))
        if [int(x) for x in metadata["padded size"]] != [Hp, Wp] or u_shape != (M, R) or v_shape != (N, R):
            raise ValueError("stream factors do not match the reflect-padded patch geometry its metadata describes")
        return C, H, W, (p, q), R
    if len(u_shape) != 3 or len(v_shape) != 3 or u_shape[0] != v_shape[0] or u_shape[2] != R or v_shape[2] != R:
        raise ValueError("stream factors are not [C, H, R] / [C, W, R]")
    C, H, W = u_shape[0], u_shape[1], v_shape[1]
    chan_dims(H, W, C, None)
    return C, H, W, None, R


def check_metrics_args(a, b, want_ssim=True):
    """The argument checks of lrf_image_metrics_u8 on two tensors, before any device is touched: TypeError for anything but
    uint8 tensors, ValueError for shapes that are not one [B,C,H,W] (B, C >= 1) or too small for the 7x7 window."""
    import torch
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError(f"image metrics take uint8 tensors, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"Input images must have the same (B, C, H, W) shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, C, H, W = a.shape
    if B < 1 or C < 1 or H < 1 or W < 1 or B > 65535:
        raise ValueError(f"shape {tuple(a.shape)} out of range")
    if want_ssim and min(H, W) < 7:
        raise ValueError("win_size exceeds image extent.")


def check_metrics_ragged_args(list_a, list_b, want_ssim=True):
    """The argument checks of lrf_image_metrics_ragged_u8 on two lists of images, before any device is touched: TypeError for
    anything but two lists of uint8 tensors, ValueError for lists that are empty, longer than 65535 or of differing lengths, for
    a pair whose shapes are not one [C,H,W] (the same C >= 1 for every pair), whose sides are below the 7x7 window (with the SSIM)
    or above 2^20, and for images that are not all on one device -> (C, [(H, W)])"""
    import torch
    for name, lst in (("list_a", list_a), ("list_b", list_b)):
        if not isinstance(lst, (list, tuple)):
            raise TypeError(f"image_metrics_ragged takes two lists of images, got {type(lst).__name__} for {name}")
        for i, t in enumerate(lst):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise TypeError(f"image_metrics_ragged: {name}[{i}] is {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}, not a uint8 tensor")
    if len(list_a) < 1 or len(list_a) > 65535 or len(list_a) != len(list_b):
        raise ValueError(f"image_metrics_ragged takes two lists of one length in [1,65535], got {len(list_a)} and {len(list_b)} images")
    sizes = []
    C = int(list_a[0].shape[0]) if list_a[0].dim() == 3 else 0
    for i, (x, y) in enumerate(zip(list_a, list_b)):
        if x.dim() != 3 or tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"image_metrics_ragged: pair {i}: both images must have one [C,H,W] shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.shape[0] != C or C < 1 or C > 65535:
            raise ValueError(f"image_metrics_ragged: pair {i} has {x.shape[0]} channels, pair 0 has {C} (every pair takes the same C in [1,65535])")
        H, W = int(x.shape[1]), int(x.shape[2])
        if min(H, W) < 1 or max(H, W) > 2 ** 20 or C * H * W >= 2 ** 40:
            raise ValueError(f"image_metrics_ragged: pair {i}: size {H}x{W} out of range")
        if want_ssim and min(H, W) < 7:
            raise ValueError(f"image_metrics_ragged: pair {i} ({H}x{W}): win_size exceeds image extent.")
        sizes.append((H, W))
    if len({t.device for t in list(list_a) + list(list_b)}) != 1:
        raise ValueError("image_metrics_ragged: the images must all be on one device")
    return C, sizes


def check_ssim_ragged_args(rgb, items, U, V, scratch_bytes=0):
    """The argument checks of lrf_qmf_ssim_ragged_rgb_u8, before any device is touched: check_sse_ragged_args', plus ValueError for
    an item with a side below the 7x7 window and for a negative scratch_bytes -> int64 array [n, 8] (the layout of _sse_items_array)"""
    a = _sse_items_array(rgb, items, U, V)
    small = (a[:, 0] < 7) | (a[:, 1] < 7)
    if small.any():
        i = int(np.nonzero(small)[0][0])
        raise ValueError(f"item {i} ({a[i, 0]}x{a[i, 1]}): win_size exceeds image extent.")
    if int(scratch_bytes) < 0:
        raise ValueError(f"scratch_bytes must be >= 0 (0: the default cap), got {scratch_bytes}")
    return a


def check_sweep_sse_args(rgb, factors, triples):
    """The argument checks of lrf_qmf_sweep_sse_rgb_u8 on its tensors, before any device is touched.  rgb: uint8 [B,3,H,W];
    triples: Q >= 1 rank triples, every rank in 1..64; factors: one (U, V) int8 pair per triple, shaped [B, sum_c M_c R_c] and
    [B, 64 sum_c R_c] for that triple (the kernel indexes the factors from (H, W) and the ranks alone: sizes that disagree would
    be out-of-bounds reads).  TypeError for anything but tensors of these types, ValueError for everything else."""
    import torch
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8:
        raise TypeError(f"sweep_sse takes a uint8 image tensor, got {rgb.dtype if isinstance(rgb, torch.Tensor) else type(rgb).__name__}")
    if rgb.dim() != 4 or rgb.shape[1] != 3 or min(rgb.shape) < 1 or rgb.shape[0] > 65535:
        raise ValueError(f"images must be [B,3,H,W] with 1 <= B <= 65535, got {tuple(rgb.shape)}")
    B, _, H, W = rgb.shape
    if factors is None or triples is None or len(triples) < 1 or len(triples) > 4096 or len(factors) != len(triples):
        raise ValueError("sweep_sse needs one (U, V) pair per rank triple, 1 to 4096 of them")
    dims = plane_dims(H, W)
    dev = None
    for t, pair in zip(triples, factors):
        if len(t) != 3 or any(int(r) != r or r < 1 or r > 64 for r in t):
            raise ValueError(f"rank triple {tuple(t)}: three ranks in 1..64 expected")
        if pair is None or len(pair) != 2 or pair[0] is None or pair[1] is None:
            raise ValueError(f"rank triple {tuple(t)}: a (U, V) pair expected")
        U, V = pair
        if not isinstance(U, torch.Tensor) or not isinstance(V, torch.Tensor) or U.dtype != torch.int8 or V.dtype != torch.int8:
            raise TypeError("factors must be int8 tensors")
        nu, nv = sum(d[4] * int(r) for d, r in zip(dims, t)), 64 * sum(int(r) for r in t)
        dev = U.device if dev is None else dev
        if tuple(U.shape) != (B, nu) or tuple(V.shape) != (B, nv) or U.device != dev or V.device != dev:
            raise ValueError(f"factor buffers do not match the geometry at ranks {tuple(t)}: expected int8 U {(B, nu)} and V {(B, nv)} on "
                             f"{dev}, got {tuple(U.shape)} on {U.device} and {tuple(V.shape)} on {V.device}")


def _check_factor_tensors(U, V, images, who):
    """what the colour and the gray image lists share: flat contiguous int8 U and V on one device, 1 to 65535 images"""
    import torch
    if not isinstance(U, torch.Tensor) or not isinstance(V, torch.Tensor) or U.dtype != torch.int8 or V.dtype != torch.int8:
        raise TypeError("factors must be int8 tensors")
    if U.dim() != 1 or V.dim() != 1 or U.device != V.device or not U.is_contiguous() or not V.is_contiguous():
        raise ValueError(f"U and V must be flat contiguous tensors on one device, got {tuple(U.shape)} on {U.device} and {tuple(V.shape)} on {V.device}")
    if images is None or len(images) < 1 or len(images) > 65535:
        raise ValueError(f"{who} needs 1 to 65535 images")


def check_ragged_args(U, V, images):
    """The argument checks of lrf_qmf_decode_ragged_rgb_u8 on its tensors, before any device is touched.  U, V: flat int8 tensors
    on one device; images: 1 to 65535 tuples (H, W, ranks, u_off, v_off), every rank in 1..64, every image's factors inside U and
    V (the kernels index them from the tuple alone: anything else would be an out-of-bounds read).  TypeError for anything but
    int8 tensors, ValueError for everything else.  -> [(H, W, [R_Y, R_Cb, R_Cr], u_off, v_off)] as integers."""
    _check_factor_tensors(U, V, images, "decode_ragged")
    out = []
    for i, im in enumerate(images):
        if len(im) != 5 or len(im[2]) != 3:
            raise ValueError(f"image {i}: (H, W, (R_Y, R_Cb, R_Cr), u_off, v_off) expected")
        H, W, ranks, u_off, v_off = im
        if any(int(x) != x for x in (H, W, u_off, v_off)) or any(int(r) != r for r in ranks):
            raise ValueError(f"image {i}: integers expected")
        H, W, u_off, v_off, ranks = int(H), int(W), int(u_off), int(v_off), [int(r) for r in ranks]
        if H < 1 or W < 1 or H >= 2 ** 31 or W >= 2 ** 31 or min(ranks) < 1 or max(ranks) > 64:
            raise ValueError(f"image {i}: size {H}x{W} or ranks {ranks} out of range (ranks 1..64)")
        dims = plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        if u_off < 0 or v_off < 0 or u_off + nu > U.numel() or v_off + nv > V.numel():
            raise ValueError(f"image {i}: its factors (U {nu} elements at {u_off}, V {nv} at {v_off}) leave the buffers of "
                             f"{U.numel()} and {V.numel()} elements")
        out.append((H, W, ranks, u_off, v_off))
    return out


def _check_size(size, upper=None):
    """The (h, w) of an entry's windows, both >= 1 — or, with `upper`, the (oh, ow) of its output, both in [1, upper] -> integers"""
    import numpy as np
    try:
        h, w = size
    except (TypeError, ValueError):
        raise ValueError(f"size must be ({'h, w' if upper is None else 'oh, ow'}), got {size!r}") from None
    if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in (h, w)):
        raise TypeError(f"size must hold two integers, got {size!r}")
    h, w = int(h), int(w)
    if upper is None and (h < 1 or w < 1):
        raise ValueError(f"crop size {h}x{w}: both sides must be >= 1")
    if upper is not None and (h < 1 or w < 1 or h > upper or w > upper):
        raise ValueError(f"output size {h}x{w}: both sides must be in [1, {upper}]")
    return h, w


def _check_boxes(crops, columns, entry, noun="crops", most=2 ** 20):
    """The box list of `entry`: an integer array-like [n, len(columns)] on the host, 1 <= n <= most (None: the caller splits the
    list and its parts are checked); columns: their names and noun: what the caller calls the list, for the messages -> an
    int64 array"""
    import numpy as np
    if hasattr(crops, "detach"):  # a torch tensor
        if crops.is_cuda:
            raise ValueError(f"{noun} live on the host: the call validates every box before it launches")
        crops = crops.detach().numpy()
    boxes = np.asarray(crops)
    if boxes.size == 0:
        raise ValueError(f"{entry} needs 1 to 2^20 crops")
    if boxes.dtype.kind not in "iu":
        raise TypeError(f"{noun} must be integers ({', '.join(columns)}), got {boxes.dtype}")
    if boxes.ndim != 2 or boxes.shape[1] != len(columns):
        raise ValueError(f"{noun} must be [n, {len(columns)}] ({', '.join(columns)}), got shape {tuple(boxes.shape)}")
    if most is not None and boxes.shape[0] > most:
        raise ValueError(f"{entry} needs 1 to 2^20 crops")
    return boxes.astype(np.int64)


def _check_box_images(boxes, ims):
    """column 0 of the boxes indexes the images -> (H, W) of every box's image"""
    import numpy as np
    bad = np.flatnonzero((boxes[:, 0] < 0) | (boxes[:, 0] >= len(ims)))
    if bad.size:
        raise ValueError(f"crop {bad[0]}: image {boxes[bad[0], 0]} out of range [0, {len(ims)})")
    return np.array([im[0] for im in ims], dtype=np.int64)[boxes[:, 0]], np.array([im[1] for im in ims], dtype=np.int64)[boxes[:, 0]]


def check_crop_args(U, V, images, crops, size):
    """The argument checks of lrf_qmf_decode_crops_rgb_u8, before any device is touched.  U, V, images: as check_ragged_args takes
    them; crops: an integer array-like [n, 3] of (image, y0, x0) on the host, 1 <= n <= 2^20; size: (h, w), both >= 1; every
    window inside its image.  TypeError for factors that are not int8 tensors and for boxes or sizes that are not integers,
    ValueError for everything else.  -> (images as check_ragged_args returns them, crops as an int32 array [n, 3], (h, w))."""
    import numpy as np
    ims = check_ragged_args(U, V, images)
    h, w = _check_size(size)
    boxes = _check_boxes(crops, ("image", "y0", "x0"), "decode_crops")
    Hs, Ws = _check_box_images(boxes, ims)
    bad = np.flatnonzero((boxes[:, 1] < 0) | (boxes[:, 2] < 0) | (boxes[:, 1] + h > Hs) | (boxes[:, 2] + w > Ws))
    if bad.size:
        j = bad[0]
        raise ValueError(f"crop {j}: {h}x{w} at ({boxes[j, 1]}, {boxes[j, 2]}) leaves image {boxes[j, 0]} of {Hs[j]}x{Ws[j]}")
    return ims, np.ascontiguousarray(boxes, dtype=np.int32), (h, w)


SCALES = (2, 4, 8)  # lrf_qmf_decode_scaled_rgb_u8


def _check_scaled_crops(ims, crops, size, scales, entry):
    """crops of (image, scale, y0, x0) against the admitted scales and the checked images `ims` (their first two fields: H, W):
    every window of `size` inside its image at its scale -> (ims, crops as an int32 array [n, 4], (h, w))"""
    import numpy as np
    h, w = _check_size(size)
    boxes = _check_boxes(crops, ("image", "scale", "y0", "x0"), entry)
    Hs, Ws = _check_box_images(boxes, ims)
    bad = np.flatnonzero(~np.isin(boxes[:, 1], scales))
    if bad.size:
        raise ValueError(f"crop {bad[0]}: scale {boxes[bad[0], 1]}: {', '.join(str(f) for f in scales[:-1])} or {scales[-1]} expected")
    f = boxes[:, 1]
    Hs, Ws = -(-Hs // f), -(-Ws // f)
    bad = np.flatnonzero((boxes[:, 2] < 0) | (boxes[:, 3] < 0) | (boxes[:, 2] + h > Hs) | (boxes[:, 3] + w > Ws))
    if bad.size:
        j = bad[0]
        raise ValueError(f"crop {j}: {h}x{w} at ({boxes[j, 2]}, {boxes[j, 3]}) leaves image {boxes[j, 0]} of {Hs[j]}x{Ws[j]} at scale 1/{f[j]}")
    return ims, np.ascontiguousarray(boxes, dtype=np.int32), (h, w)


def scaled_dims(H, W, scale):
    """(ceil(H / scale), ceil(W / scale)): the size of an H x W image decoded at 1/scale (lrf_scaled_dims)"""
    if isinstance(scale, bool) or int(scale) != scale or int(scale) not in SCALES:
        raise ValueError(f"scale {scale!r}: 2, 4 or 8 expected")
    if H < 1 or W < 1:
        raise ValueError(f"size {H}x{W} out of range")
    scale = int(scale)
    return -(-int(H) // scale), -(-int(W) // scale)


def check_scaled_args(U, V, images, scale=None, crops=None, size=None):
    """The argument checks of lrf_qmf_decode_scaled_rgb_u8 (scale: 2, 4 or 8; crops and size None) and of
    lrf_qmf_decode_scaled_crops_rgb_u8 (scale None; crops: an integer array-like [n, 4] of (image, scale, y0, x0) on the host,
    1 <= n <= 2^20, y0 and x0 in the scaled image; size: (h, w), both >= 1; every window inside its image's scaled size), before
    any device is touched.  U, V, images: as check_ragged_args takes them.  TypeError for factors that are not int8 tensors and
    for scales, boxes or sizes that are not integers, ValueError for everything else.
    -> (images as check_ragged_args returns them, scale) or (images, crops as an int32 array [n, 4], (h, w))."""
    import numpy as np
    ims = check_ragged_args(U, V, images)
    if crops is None and size is None:
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)):
            raise TypeError(f"scale must be an integer, got {scale!r}")
        if int(scale) not in SCALES:
            raise ValueError(f"scale {scale}: 2, 4 or 8 expected")
        return ims, int(scale)
    if scale is not None or crops is None or size is None:
        raise ValueError("give either a scale (whole images) or crops of (image, scale, y0, x0) and a size")
    return _check_scaled_crops(ims, crops, size, SCALES, "decode_scaled_crops")


RESIZED_MAX_SIDE = 16384  # lrf_qmf_decode_resized_crops_rgb_u8: the largest output side


def _check_resized_boxes(ims, crops, size):
    """boxes of (image, y0, x0, h, w, flip) against the checked images `ims` (their first two fields: H, W) and the output size
    -> (ims, crops as an int32 array [n, 6] with flip 0 or 1, (oh, ow))"""
    import numpy as np
    oh, ow = _check_size(size, RESIZED_MAX_SIDE)
    boxes = _check_boxes(crops, ("image", "y0", "x0", "h", "w", "flip"), "decode_resized_crops")
    Hs, Ws = _check_box_images(boxes, ims)
    bad = np.flatnonzero((boxes[:, 3] < 1) | (boxes[:, 4] < 1))
    if bad.size:
        raise ValueError(f"crop {bad[0]}: box of {boxes[bad[0], 3]}x{boxes[bad[0], 4]}: both sides must be >= 1")
    bad = np.flatnonzero((boxes[:, 1] < 0) | (boxes[:, 2] < 0) | (boxes[:, 1] + boxes[:, 3] > Hs) | (boxes[:, 2] + boxes[:, 4] > Ws))
    if bad.size:
        j = bad[0]
        raise ValueError(f"crop {j}: {boxes[j, 3]}x{boxes[j, 4]} at ({boxes[j, 1]}, {boxes[j, 2]}) leaves image {boxes[j, 0]} of {Hs[j]}x{Ws[j]}")
    boxes[:, 5] = boxes[:, 5] != 0
    return ims, np.ascontiguousarray(boxes, dtype=np.int32), (oh, ow)


def check_resized_args(U, V, images, crops, size):
    """The argument checks of lrf_qmf_decode_resized_crops_rgb_u8, before any device is touched.  U, V, images: as
    check_ragged_args takes them; crops: an integer array-like [n, 6] of (image, y0, x0, h, w, flip) on the host, 1 <= n <= 2^20,
    h and w >= 1, every box inside its image; size: (oh, ow), both in [1, 16384].  TypeError for factors that are not int8
    tensors and for boxes or sizes that are not integers, ValueError for everything else.
    -> (images as check_ragged_args returns them, crops as an int32 array [n, 6] with flip 0 or 1, (oh, ow))."""
    return _check_resized_boxes(check_ragged_args(U, V, images), crops, size)


T_F32, T_F16, T_BF16 = 0, 1, 2  # lrf_tensor_format.dtype
T_NCHW, T_NHWC = 0, 1  # lrf_tensor_format.layout


def _three_numbers(v, name):
    """None, one number or three of them -> three Python floats, or None"""
    import numpy as np
    if v is None:
        return None
    number = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))
    if number(v):
        return [float(v)] * 3
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or not hasattr(v, "__getitem__"):
        raise TypeError(f"{name} must be None, a number or three numbers, got {v!r}")
    if hasattr(v, "tolist"):
        v = v.tolist()
    if not isinstance(v, (list, tuple)) or not all(number(x) for x in v):
        raise TypeError(f"{name} must be None, a number or three numbers, got {v!r}")
    if len(v) != 3:
        raise ValueError(f"{name} must hold one value per channel (3), got {len(v)}")
    return [float(x) for x in v]


def check_tensor_format(dtype, mean=None, std=None, channels_last=False):
    """The tensor format of the model-ready decode entries (lrf_tensor_format, include/lrf_hip.h), before any device is touched.
    dtype: torch.float32, float16 or bfloat16; mean, std: None, one number or three, in [0, 1] units as torchvision's Normalize
    after ToDtype(scale=True); channels_last: NHWC memory.  scale[k] = float32(1 / (255 std[k])), bias[k] = float32(-mean[k] /
    std[k]), each computed in Python doubles and rounded once; without mean and std float32(1 / 255) and 0.  TypeError for
    anything of the wrong type, ValueError for a std of 0, for values that are not finite (as float32 too) and for a wrong count.
    -> TensorFormat"""
    import math
    import numpy as np
    import torch
    if not isinstance(dtype, torch.dtype):
        raise TypeError(f"dtype must be a torch.dtype, got {dtype!r}")
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"dtype {dtype}: torch.float32, torch.float16 or torch.bfloat16 expected")
    if not isinstance(channels_last, (bool, np.bool_)):
        raise TypeError(f"channels_last must be a bool, got {channels_last!r}")
    m, s = _three_numbers(mean, "mean"), _three_numbers(std, "std")
    m, s = m if m is not None else [0.0] * 3, s if s is not None else [1.0] * 3
    if not all(math.isfinite(x) for x in m + s):
        raise ValueError(f"mean and std must be finite, got {mean!r} and {std!r}")
    if any(x == 0.0 for x in s):
        raise ValueError(f"std must not contain 0, got {std!r}")
    fmt = TensorFormat()
    fmt.dtype = {torch.float32: T_F32, torch.float16: T_F16, torch.bfloat16: T_BF16}[dtype]
    fmt.layout = T_NHWC if channels_last else T_NCHW
    for k in range(3):
        with np.errstate(over="ignore"):
            sc, bi = np.float32(1.0 / (255.0 * s[k])), np.float32(-m[k] / s[k])
        if not (np.isfinite(sc) and np.isfinite(bi)):
            raise ValueError(f"channel {k}: scale {sc} or bias {bi} is not a finite float32 (mean {m[k]}, std {s[k]})")
        fmt.scale[k], fmt.bias[k] = float(sc), float(bi)
    return fmt


def _tensor_request(entry, dtype, mean, std, channels_last, out, channels=3):
    """The output arguments the decode entries share, checked before any device is touched -> None for the uint8 entry (the
    defaults), else the TensorFormat.  channels 1 (the gray loader): mean and std are None, one number or a sequence of one (three
    numbers: ValueError), and only element 0 of the format's scale and bias is read"""
    import torch
    if dtype == torch.uint8:
        if mean is not None or std is not None or channels_last or out is not None:
            raise ValueError(f"{entry}: mean, std, channels_last and out= go with a float dtype (dtype=torch.uint8 is the byte entry, [n,{channels},h,w])")
        return None
    if channels == 1:
        mean, std = _one_number(mean, "mean"), _one_number(std, "std")
    return check_tensor_format(dtype, mean, std, channels_last)


def _tensor_output(entry, out, n, h, w, dtype, channels_last, device, channels=3):
    """the [n,channels,h,w] result of a tensor entry: the caller's `out`, checked (a refusal launches nothing), or a new tensor.
    With one channel NCHW and channels_last are the same memory: n images of h w elements, rows of w ("dense")"""
    import torch
    C, channels_last = channels, channels_last and channels > 1
    if out is None:
        return torch.empty((n, C, h, w), dtype=dtype, device=device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{entry}: out must be a tensor, got {type(out).__name__}")
    if out.dtype != dtype or tuple(out.shape) != (n, C, h, w) or out.device != device:
        raise ValueError(f"{entry}: out must be {dtype} {(n, C, h, w)} on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    # (strides, not is_contiguous(memory_format=...): for h = w = 1 or n = 1 torch calls more than one layout contiguous; the
    # stride of an axis of size 1 — the channel axis of a gray tensor — is immaterial)
    want = (C * h * w, 1, C * w, C) if channels_last else (C * h * w, h * w, w, 1)
    if any(st != wt for st, wt, size in zip(out.stride(), want, out.shape) if size > 1):
        memory = "channels_last" if channels_last else ("contiguous" if C > 1 else "dense")
        raise ValueError(f"{entry}: out must be {memory} memory (strides {want}), got strides {tuple(out.stride())}")
    return out


GRAY_SCALES = (1, 2, 4, 8)  # the levels of the gray loader (lrf_qmf_decode_gray_ragged_u8, lrf_qmf_decode_gray_crops_u8)


def check_gray_images(U, V, images):
    """The image list of the gray loader (lrf_gray_image), before any device is touched.  U, V: flat int8 tensors on one device;
    images: 1 to 65535 tuples (H, W, R, u_off, v_off), R one rank in 1..64, the image's U [M, R] and V [64, R] inside U and V, M
    from lrf_chan_dims(H, W, 1, 8, 8) (which refuses sizes the decoder refuses).  TypeError for anything but int8 tensors,
    ValueError for everything else.  -> [(H, W, R, u_off, v_off)] as integers."""
    _check_factor_tensors(U, V, images, "the gray loader")
    out = []
    for i, im in enumerate(images):
        if len(im) != 5 or hasattr(im[2], "__len__"):
            raise ValueError(f"image {i}: (H, W, R, u_off, v_off) expected")
        if any(int(x) != x for x in im):
            raise ValueError(f"image {i}: integers expected")
        H, W, R, u_off, v_off = (int(x) for x in im)
        if H < 1 or W < 1 or H * W >= 2 ** 31 or R < 1 or R > 64:
            raise ValueError(f"image {i}: size {H}x{W} or rank {R} out of range (rank 1..64, fewer than 2^31 pixels)")
        M = chan_dims(H, W, 1, (8, 8))[2]
        if u_off < 0 or v_off < 0 or u_off + M * R > U.numel() or v_off + 64 * R > V.numel():
            raise ValueError(f"image {i}: its factors (U {M * R} elements at {u_off}, V {64 * R} at {v_off}) leave the buffers of "
                             f"{U.numel()} and {V.numel()} elements")
        out.append((H, W, R, u_off, v_off))
    return out


def gray_scaled_dims(H, W, scale):
    """(ceil(H / scale), ceil(W / scale)) for scale 1, 2, 4, 8"""
    if isinstance(scale, bool) or int(scale) != scale or int(scale) not in GRAY_SCALES:
        raise ValueError(f"scale {scale!r}: 1, 2, 4 or 8 expected")
    return -(-int(H) // int(scale)), -(-int(W) // int(scale))


def check_gray_scale(scale):
    """the level of a whole-image decode of the gray loader: TypeError unless an integer, ValueError unless 1, 2, 4 or 8 -> int"""
    import numpy as np
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)):
        raise TypeError(f"scale must be an integer, got {scale!r}")
    if int(scale) not in GRAY_SCALES:
        raise ValueError(f"scale {scale}: 1, 2, 4 or 8 expected")
    return int(scale)


def check_gray_crop_args(U, V, images, crops, size):
    """The argument checks of lrf_qmf_decode_gray_crops_u8, before any device is touched.  U, V, images: as check_gray_images takes
    them; crops: an integer array-like [n, 4] of (image, scale, y0, x0) on the host, 1 <= n <= 2^20, the scale per crop out of 1,
    2, 4, 8 and y0, x0 in the image at that scale; size: (h, w), both >= 1; every window inside its image's scaled size.
    -> (images, crops as an int32 array [n, 4], (h, w))."""
    return _check_scaled_crops(check_gray_images(U, V, images), crops, size, GRAY_SCALES, "decode_crops")


def check_gray_resized_args(U, V, images, crops, size):
    """The argument checks of lrf_qmf_decode_gray_resized_crops_u8, before any device is touched: check_resized_args for a gray
    image list (check_gray_images) -> (images, crops as an int32 array [n, 6] with flip 0 or 1, (oh, ow))."""
    return _check_resized_boxes(check_gray_images(U, V, images), crops, size)


def _one_number(v, name):
    """None, one number or a sequence of one -> that number for check_tensor_format, or None; three numbers (a colour triple) and
    any other count: ValueError"""
    if v is None or not hasattr(v, "__len__") or isinstance(v, (str, bytes)):
        return v  # (a scalar, or a type check_tensor_format refuses)
    if hasattr(v, "tolist"):
        v = v.tolist()
    if not isinstance(v, (list, tuple)):
        return v
    if len(v) != 1:
        raise ValueError(f"{name} of a gray image must hold one value (one channel), got {len(v)}")
    return v[0]


def check_gray_tensor_request(entry, dtype, mean, std, channels_last, out):
    """_tensor_request for the gray loader -> None for the uint8 entry, else the TensorFormat"""
    return _tensor_request(entry, dtype, mean, std, channels_last, out, channels=1)


def _gray_tensor_output(entry, out, n, h, w, dtype, device):
    """_tensor_output for the gray loader: the [n,1,h,w] result, the caller's dense `out` or a new tensor"""
    return _tensor_output(entry, out, n, h, w, dtype, False, device, channels=1)


def _gray_images(ims, out_offs=None):
    """the lrf_gray_image array of a checked image list (check_gray_images); out_offs: where each image's output starts, else 0"""
    desc = (GrayImage * len(ims))()
    for i, (d, (H, W, R, u_off, v_off)) in enumerate(zip(desc, ims)):
        d.H, d.W, d.R, d.u_off, d.v_off, d.out_off = H, W, R, u_off, v_off, 0 if out_offs is None else out_offs[i]
    return desc


def _check_gray_pixels(entry, gray, sign):
    import torch
    if not isinstance(gray, torch.Tensor) or gray.dtype != torch.uint8:
        raise TypeError(f"{entry} takes its pixels as a uint8 tensor")
    if sign is not None and (not isinstance(sign, torch.Tensor) or sign.dtype != torch.int8):
        raise TypeError(f"{entry} takes its signs as an int8 tensor")
    if gray.dim() != 1 or not gray.is_contiguous() or (sign is not None and (sign.dim() != 1 or not sign.is_contiguous() or sign.device != gray.device)):
        raise ValueError("gray (and sign) must be flat contiguous tensors on one device")


def _check_gray_rank(who, R):
    if isinstance(R, bool) or hasattr(R, "__len__") or int(R) != R:
        raise ValueError(f"{who}: one integer rank expected (a gray stream has a scalar rank), got {R!r}")
    if int(R) < 1 or int(R) > 32:
        raise ValueError(f"{who}: rank {int(R)} out of range (1..32)")
    return int(R)


def _check_gray_source(i, im, gray, lead):
    """(H, W, gray_off, sign_off) of the image tuple whose first `lead` + 1 fields are H, W[, R], gray_off, then an optional sign_off"""
    H, W, gray_off = im[0], im[1], im[lead]
    sign_off = im[lead + 1] if len(im) == lead + 2 and im[lead + 1] is not None else -1
    if any(isinstance(x, bool) or int(x) != x for x in (H, W, gray_off, sign_off)):
        raise ValueError(f"image {i}: integers expected")
    H, W, gray_off, sign_off = int(H), int(W), int(gray_off), int(sign_off)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"image {i}: size {H}x{W} out of range (fewer than 2^31 pixels)")
    chan_dims(H, W, 1, (8, 8))  # (refuses what the encoder refuses)
    if gray_off < 0 or gray_off + H * W > gray.numel():
        raise ValueError(f"image {i}: its {H * W} bytes at {gray_off} leave the buffer of {gray.numel()} bytes")
    return H, W, gray_off, sign_off


def _check_gray_signs(i, sign_off, R, sign):
    if sign_off < -1 or (sign_off >= 0 and (sign is None or sign_off + R > sign.numel())):
        raise ValueError(f"image {i}: its {R} signs at {sign_off} leave the sign buffer")


def check_encode_gray_ragged_args(gray, images, sign=None):
    """The argument checks of lrf_qmf_encode_gray_ragged_u8 on its tensors, before any device is touched.  gray: a flat uint8
    tensor; images: 1 to 65535 tuples (H, W, R, gray_off[, sign_off]) with R one rank in 1..32 and every image's [H, W] bytes
    inside gray; sign: None or a flat int8 tensor on gray's device, an image's sign_off (-1 or absent: the default signs) naming
    where its R signs start.  TypeError for tensors of another type, ValueError for everything else.
    -> [(H, W, R, gray_off, sign_off)] as integers."""
    _check_gray_pixels("encode_gray_ragged", gray, sign)
    if images is None or len(images) < 1 or len(images) > 65535:
        raise ValueError("encode_gray_ragged needs 1 to 65535 images")
    out = []
    for i, im in enumerate(images):
        if not hasattr(im, "__len__") or len(im) not in (4, 5):
            raise ValueError(f"image {i}: (H, W, R, gray_off[, sign_off]) expected")
        R = _check_gray_rank(f"image {i}", im[2])
        H, W, gray_off, sign_off = _check_gray_source(i, im, gray, 3)
        _check_gray_signs(i, sign_off, R, sign)
        out.append((H, W, R, gray_off, sign_off))
    return out


def check_encode_gray_ragged_sweep_args(gray, images, cands, sign=None):
    """The argument checks of lrf_qmf_encode_gray_ragged_sweep_u8 on its tensors, before any device is touched.  gray: a flat
    uint8 tensor; images: 1 to 65535 tuples (H, W, gray_off[, sign_off]); cands: up to 2^20 tuples (image, R), R in 1..32, at
    least one per image, in any order; sign: None or a flat int8 tensor on gray's device, an image's sign_off (-1 or absent: the
    default signs) naming where its signs start — as many as its largest candidate rank.  TypeError for tensors of another
    type, ValueError for everything else.  -> ([(H, W, gray_off, sign_off)], [(image, R)]) as integers."""
    _check_gray_pixels("encode_gray_ragged_sweep", gray, sign)
    if images is None or len(images) < 1 or len(images) > 65535:
        raise ValueError("encode_gray_ragged_sweep needs 1 to 65535 images")
    if cands is None or len(cands) < len(images) or len(cands) > 2 ** 20:
        raise ValueError(f"encode_gray_ragged_sweep needs a candidate per image at least and 2^20 at most, got {0 if cands is None else len(cands)} for {len(images)} images")
    ims = []
    for i, im in enumerate(images):
        if not hasattr(im, "__len__") or len(im) not in (3, 4):
            raise ValueError(f"image {i}: (H, W, gray_off[, sign_off]) expected")
        ims.append(_check_gray_source(i, im, gray, 2))
    rmax, cds = [0] * len(ims), []
    for j, cd in enumerate(cands):
        if not hasattr(cd, "__len__") or len(cd) != 2:
            raise ValueError(f"candidate {j}: (image, R) expected")
        if isinstance(cd[0], bool) or int(cd[0]) != cd[0] or int(cd[0]) < 0 or int(cd[0]) >= len(ims):
            raise ValueError(f"candidate {j}: image {cd[0]!r} out of range [0,{len(ims)})")
        R = _check_gray_rank(f"candidate {j}", cd[1])
        rmax[int(cd[0])] = max(rmax[int(cd[0])], R)
        cds.append((int(cd[0]), R))
    for i, (r, im) in enumerate(zip(rmax, ims)):
        if r == 0:
            raise ValueError(f"image {i} has no candidate")
        _check_gray_signs(i, im[3], r, sign)
    return ims, cds


def check_sse_gray_ragged_args(gray, items, U, V):
    """The argument checks of lrf_qmf_sse_gray_ragged_u8 on its tensors, before any device is touched.  gray: a flat uint8 tensor
    holding the sources; U, V: flat int8 tensors on its device; items: 1 to 65535 tuples (H, W, R, u_off, v_off, gray_off), R in
    1..64, the factors inside U and V (check_gray_images) and the [H, W] source inside gray (sources may be shared).  TypeError
    for tensors of another type, ValueError for everything else.  -> [(H, W, R, u_off, v_off, gray_off)] as integers."""
    import torch
    if not isinstance(gray, torch.Tensor) or gray.dtype != torch.uint8:
        raise TypeError("sse_gray_ragged takes its sources as a uint8 tensor")
    if gray.dim() != 1 or not gray.is_contiguous():
        raise ValueError("sse_gray_ragged takes its sources as a flat contiguous tensor")
    if items is not None and any(not hasattr(it, "__len__") or len(it) != 6 for it in items):
        raise ValueError("items: (H, W, R, u_off, v_off, gray_off) expected")
    ims = check_gray_images(U, V, None if items is None else [it[:5] for it in items])
    if U.device != gray.device:
        raise ValueError(f"sse_gray_ragged needs its tensors on one device, got {gray.device} and {U.device}")
    out = []
    for i, (im, it) in enumerate(zip(ims, items)):
        if isinstance(it[5], bool) or int(it[5]) != it[5]:
            raise ValueError(f"item {i}: integers expected")
        off = int(it[5])
        if off < 0 or off + im[0] * im[1] > gray.numel():
            raise ValueError(f"item {i}: its source of {im[0] * im[1]} bytes at {off} leaves the buffer of {gray.numel()} bytes")
        out.append(im + (off,))
    return out


def check_encode_ragged_args(rgb, images, sign=None):
    """The argument checks of lrf_qmf_encode_ragged_rgb_u8 on its tensors, before any device is touched.  rgb: a flat uint8 tensor;
    images: 1 to 65535 tuples (H, W, ranks, rgb_off[, sign_off]) with every rank in 1..32 and every image's bytes inside rgb (the
    kernels index them from the tuple alone); sign: None or a flat int8 tensor on rgb's device, an image's sign_off (-1 or absent:
    the default signs) naming where its sum(ranks) signs start.  TypeError for tensors of another type, ValueError for everything
    else.  -> [(H, W, [R_Y, R_Cb, R_Cr], rgb_off, sign_off)] as integers."""
    import torch
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8:
        raise TypeError("encode_ragged takes its pixels as a uint8 tensor")
    if sign is not None and (not isinstance(sign, torch.Tensor) or sign.dtype != torch.int8):
        raise TypeError("encode_ragged takes its signs as an int8 tensor")
    if rgb.dim() != 1 or not rgb.is_contiguous() or (sign is not None and (sign.dim() != 1 or not sign.is_contiguous() or sign.device != rgb.device)):
        raise ValueError("rgb (and sign) must be flat contiguous tensors on one device")
    if images is None or len(images) < 1 or len(images) > 65535:
        raise ValueError("encode_ragged needs 1 to 65535 images")
    out = []
    for i, im in enumerate(images):
        if len(im) not in (4, 5) or len(im[2]) != 3:
            raise ValueError(f"image {i}: (H, W, (R_Y, R_Cb, R_Cr), rgb_off[, sign_off]) expected")
        H, W, ranks, rgb_off = im[:4]
        sign_off = im[4] if len(im) == 5 and im[4] is not None else -1
        if any(int(x) != x for x in (H, W, rgb_off, sign_off)) or any(int(r) != r for r in ranks):
            raise ValueError(f"image {i}: integers expected")
        H, W, rgb_off, sign_off, ranks = int(H), int(W), int(rgb_off), int(sign_off), [int(r) for r in ranks]
        if H < 1 or W < 1 or 3 * H * W >= 2 ** 31 or min(ranks) < 1 or max(ranks) > 32:
            raise ValueError(f"image {i}: size {H}x{W} or ranks {ranks} out of range (ranks 1..32, fewer than 2^31 / 3 pixels)")
        if rgb_off < 0 or rgb_off + 3 * H * W > rgb.numel():
            raise ValueError(f"image {i}: its {3 * H * W} bytes at {rgb_off} leave the buffer of {rgb.numel()} bytes")
        if sign_off < -1 or (sign_off >= 0 and (sign is None or sign_off + sum(ranks) > sign.numel())):
            raise ValueError(f"image {i}: its {sum(ranks)} signs at {sign_off} leave the sign buffer")
        out.append((H, W, ranks, rgb_off, sign_off))
    return out


def _check_encode_ragged_sweep(rgb, images, cands, sign=None):
    """The argument checks of lrf_qmf_encode_ragged_sweep_rgb_u8 on its tensors, before any device is touched.  rgb: a flat uint8
    tensor; images: 1 to 65535 tuples (H, W, rgb_off[, sign_off]) with every image's bytes inside rgb; cands: up to 2^20 tuples
    (image, ranks), every rank in 1..32, at least one per image, in any order; sign: None or a flat int8 tensor on rgb's device,
    an image's sign_off (-1 or absent: the default signs) naming where its signs start — one per channel's largest rank over the
    image's candidates.  TypeError for tensors of another type, ValueError for everything else.
    -> ([(H, W, rgb_off, sign_off)], int64 array [m, 4] of (image, R_Y, R_Cb, R_Cr)); the candidates may be given as such an array."""
    import torch
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8:
        raise TypeError("encode_ragged_sweep takes its pixels as a uint8 tensor")
    if sign is not None and (not isinstance(sign, torch.Tensor) or sign.dtype != torch.int8):
        raise TypeError("encode_ragged_sweep takes its signs as an int8 tensor")
    if rgb.dim() != 1 or not rgb.is_contiguous() or (sign is not None and (sign.dim() != 1 or not sign.is_contiguous() or sign.device != rgb.device)):
        raise ValueError("rgb (and sign) must be flat contiguous tensors on one device")
    if images is None or len(images) < 1 or len(images) > 65535:
        raise ValueError("encode_ragged_sweep needs 1 to 65535 images")
    if cands is None or len(cands) < len(images) or len(cands) > 2 ** 20:
        raise ValueError(f"encode_ragged_sweep needs a candidate per image at least and 2^20 at most, got {0 if cands is None else len(cands)} for {len(images)} images")
    ims = []
    for i, im in enumerate(images):
        if len(im) not in (3, 4):
            raise ValueError(f"image {i}: (H, W, rgb_off[, sign_off]) expected")
        H, W, rgb_off = im[:3]
        sign_off = im[3] if len(im) == 4 and im[3] is not None else -1
        if any(int(x) != x for x in (H, W, rgb_off, sign_off)):
            raise ValueError(f"image {i}: integers expected")
        H, W, rgb_off, sign_off = int(H), int(W), int(rgb_off), int(sign_off)
        if H < 1 or W < 1 or 3 * H * W >= 2 ** 31:
            raise ValueError(f"image {i}: size {H}x{W} out of range (fewer than 2^31 / 3 pixels)")
        if rgb_off < 0 or rgb_off + 3 * H * W > rgb.numel():
            raise ValueError(f"image {i}: its {3 * H * W} bytes at {rgb_off} leave the buffer of {rgb.numel()} bytes")
        ims.append((H, W, rgb_off, sign_off))
    ims_a = np.array(ims, dtype=np.int64).reshape(-1, 4)
    cds = _sweep_candidates_array(cands, len(ims))
    rmax = np.zeros((len(ims), 3), dtype=np.int64)
    np.maximum.at(rmax, cds[:, 0], cds[:, 1:4])
    none = np.nonzero(rmax[:, 0] == 0)[0]
    if none.size:
        raise ValueError(f"image {int(none[0])} has no candidate")
    bad = (ims_a[:, 3] < -1) | ((ims_a[:, 3] >= 0) & ((sign is None) | (ims_a[:, 3] + rmax.sum(axis=1) > (0 if sign is None else sign.numel()))))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"image {i}: its {int(rmax[i].sum())} signs at {int(ims_a[i, 3])} leave the sign buffer")
    return ims, cds


def check_encode_ragged_sweep_args(rgb, images, cands, sign=None):
    """_check_encode_ragged_sweep with the candidates as a list: ([(H, W, rgb_off, sign_off)], [(image, [R_Y, R_Cb, R_Cr])])"""
    ims, cds = _check_encode_ragged_sweep(rgb, images, cands, sign)
    return ims, [(c[0], c[1:]) for c in cds.tolist()]


def _sweep_candidates_array(cands, n_images):
    """[(image, (R_Y, R_Cb, R_Cr))] -> int64 array [m, 4], checked as a whole (ValueError names the first offender)"""
    if isinstance(cands, np.ndarray) and cands.ndim == 2 and cands.shape[1] == 4:  # (image, R_Y, R_Cb, R_Cr) per row
        raw = cands
    else:
        try:
            flat = [(cd[0], cd[1][0], cd[1][1], cd[1][2]) for cd in cands if len(cd) == 2 and len(cd[1]) == 3]
        except TypeError:
            flat = []
        if len(flat) != len(cands):
            j = next(j for j, cd in enumerate(cands) if not (hasattr(cd, "__len__") and len(cd) == 2 and hasattr(cd[1], "__len__") and len(cd[1]) == 3))
            raise ValueError(f"candidate {j}: (image, (R_Y, R_Cb, R_Cr)) expected")
        raw = np.array(flat)
    if raw.dtype.kind not in "iu":
        if raw.dtype.kind != "f" or not np.array_equal(raw, np.floor(raw)):
            raise ValueError("candidates: integers expected")
    cds = raw.astype(np.int64).reshape(-1, 4)
    bad = (cds[:, 0] < 0) | (cds[:, 0] >= n_images)
    if bad.any():
        j = int(np.nonzero(bad)[0][0])
        raise ValueError(f"candidate {j}: image {int(cds[j, 0])} out of range [0,{n_images})")
    bad = (cds[:, 1:].min(axis=1) < 1) | (cds[:, 1:].max(axis=1) > 32)
    if bad.any():
        j = int(np.nonzero(bad)[0][0])
        raise ValueError(f"candidate {j}: ranks {cds[j, 1:].tolist()} out of range (1..32)")
    return cds


def _sse_items_array(rgb, items, U, V):
    """check_sse_ragged_args on the whole list at once -> int64 array [n, 8] of (H, W, R_Y, R_Cb, R_Cr, u_off, v_off, rgb_off)"""
    import torch
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8:
        raise TypeError("sse_ragged takes its sources as a uint8 tensor")
    if not isinstance(U, torch.Tensor) or not isinstance(V, torch.Tensor) or U.dtype != torch.int8 or V.dtype != torch.int8:
        raise TypeError("factors must be int8 tensors")
    if rgb.dim() != 1 or not rgb.is_contiguous():
        raise ValueError("sse_ragged takes its sources as a flat contiguous tensor")
    if U.dim() != 1 or V.dim() != 1 or U.device != V.device or not U.is_contiguous() or not V.is_contiguous():
        raise ValueError(f"U and V must be flat contiguous tensors on one device, got {tuple(U.shape)} on {U.device} and {tuple(V.shape)} on {V.device}")
    if U.device != rgb.device:
        raise ValueError(f"sse_ragged needs its tensors on one device, got {rgb.device} and {U.device}")
    if isinstance(items, np.ndarray) and items.ndim == 2 and items.shape[1] == 8 and items.dtype.kind in "iu":
        a = items.astype(np.int64, copy=False)
    else:
        if items is None or len(items) < 1:
            raise ValueError("sse_ragged needs at least one item")
        try:
            flat = [(it[0], it[1], it[2][0], it[2][1], it[2][2], it[3], it[4], it[5]) for it in items if len(it) == 6 and len(it[2]) == 3]
        except TypeError:
            flat = []
        if len(flat) != len(items):
            i = next(i for i, it in enumerate(items) if not (hasattr(it, "__len__") and len(it) == 6 and hasattr(it[2], "__len__") and len(it[2]) == 3))
            raise ValueError(f"item {i}: (H, W, (R_Y, R_Cb, R_Cr), u_off, v_off, rgb_off) expected")
        raw = np.array(flat)
        if raw.dtype.kind not in "iu" and (raw.dtype.kind != "f" or not np.array_equal(raw, np.floor(raw))):
            raise ValueError("items: integers expected")
        a = raw.astype(np.int64).reshape(-1, 8)
    if a.shape[0] < 1:
        raise ValueError("sse_ragged needs at least one item")

    def first(bad, what):
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"item {i}: {what(i)}")
    first((a[:, 0] < 1) | (a[:, 1] < 1) | (a[:, 0] >= 2 ** 31) | (a[:, 1] >= 2 ** 31) | (a[:, 2:5].min(axis=1) < 1) | (a[:, 2:5].max(axis=1) > 64),
          lambda i: f"size {a[i, 0]}x{a[i, 1]} or ranks {a[i, 2:5].tolist()} out of range (ranks 1..64)")
    Ms = plane_patches(a[:, 0], a[:, 1])
    nu, nv, px = (Ms * a[:, 2:5]).sum(axis=1), 64 * a[:, 2:5].sum(axis=1), 3 * a[:, 0] * a[:, 1]
    first((a[:, 5] < 0) | (a[:, 6] < 0) | (a[:, 5] > U.numel() - nu) | (a[:, 6] > V.numel() - nv),
          lambda i: f"its factors (U {nu[i]} elements at {a[i, 5]}, V {nv[i]} at {a[i, 6]}) leave the buffers of {U.numel()} and {V.numel()} elements")
    first((a[:, 7] < 0) | (a[:, 7] > rgb.numel() - px), lambda i: f"its source of {px[i]} bytes at {a[i, 7]} leaves the buffer of {rgb.numel()} bytes")
    return a


def check_sse_ragged_args(rgb, items, U, V):
    """The argument checks of lrf_qmf_sse_ragged_rgb_u8 on its tensors, before any device is touched.  rgb: a flat uint8 tensor
    holding the sources; U, V: flat int8 tensors on its device; items: at least one tuple (H, W, ranks, u_off, v_off, rgb_off) — or
    an integer array [n, 8] of (H, W, R_Y, R_Cb, R_Cr, u_off, v_off, rgb_off) — every rank in 1..64, the factors inside U and V and
    the [3,H,W] source inside rgb (sources may be shared).  The list is checked as a whole, the geometry asked once per distinct
    size.  TypeError for tensors of another type, ValueError for everything else.
    -> [(H, W, [R_Y, R_Cb, R_Cr], u_off, v_off, rgb_off)] as integers."""
    return [(r[0], r[1], r[2:5], r[5], r[6], r[7]) for r in _sse_items_array(rgb, items, U, V).tolist()]


def deflate_bound(length):
    """bytes of the slot a column of `length` bytes gets: 2 + 5 * ceil(length / 65535) + length + 4 (host-only arithmetic; works
    on integers and on integer arrays alike)"""
    return 2 + 5 * ((length + 65534) // 65535) + length + 4


def deflate_table(mats):
    """The table lrf_deflate_columns_i8 takes, as an int64 array [n, 5] of (src_off, rows, cols, dst_off, len_off), from an
    integer array-like [n, 3] of (src_off, rows, cols): slots and length entries back to back in call order -> (table, bytes
    of all slots, number of columns).  Host-only arithmetic."""
    m = np.asarray(mats, dtype=np.int64).reshape(-1, 3)
    if m.shape[0] < 1 or bool((m[:, 1:] < 1).any()) or bool((m[:, 0] < 0).any()):
        raise ValueError("deflate_columns needs at least one matrix (src_off >= 0, rows >= 1, cols >= 1)")
    slots = m[:, 2] * deflate_bound(m[:, 1])
    table = np.empty((m.shape[0], 5), dtype=np.int64)
    table[:, :3] = m
    table[:, 3] = np.cumsum(slots) - slots
    table[:, 4] = np.cumsum(m[:, 2]) - m[:, 2]
    return table, int(slots.sum()), int(m[:, 2].sum())


def deflate_column_offsets(table):
    """per column of a table (deflate_table's layout) where its slot starts: int64 [number of columns], matrices in table order"""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 5)
    cols = t[:, 2]
    first = np.cumsum(cols) - cols
    within = np.arange(int(cols.sum()), dtype=np.int64) - np.repeat(first, cols)
    return np.repeat(t[:, 3], cols) + within * np.repeat(deflate_bound(t[:, 1]), cols)


def inflate_table(mats):
    """The table lrf_inflate_columns_i8 takes, as an int64 array [n, 4] of (dst_off, rows, cols, first), from an integer
    array-like [n, 2] of (rows, cols): the matrices back to back in the destination and their streams in call order -> (table,
    bytes of all matrices, number of columns).  Host-only arithmetic."""
    m = np.asarray(mats, dtype=np.int64).reshape(-1, 2)
    if m.shape[0] < 1 or bool((m < 1).any()):
        raise ValueError("inflate_columns needs at least one matrix (rows >= 1, cols >= 1)")
    size = m[:, 0] * m[:, 1]
    table = np.empty((m.shape[0], 4), dtype=np.int64)
    table[:, 0] = np.cumsum(size) - size
    table[:, 1:3] = m
    table[:, 3] = np.cumsum(m[:, 1]) - m[:, 1]
    return table, int(size.sum()), int(m[:, 1].sum())


def flat_views(ts):
    """One flat tensor holding the int8 tensors `ts` back to back (the C layout of a sweep: triple after triple): where they
    already are consecutive views of one buffer, as encode_sweep_rgb returns them, a view of it; a copy otherwise."""
    import torch
    p = ts[0].data_ptr()
    for t in ts:
        if not t.is_contiguous() or t.data_ptr() != p or t.untyped_storage().data_ptr() != ts[0].untyped_storage().data_ptr():
            return torch.cat([x.reshape(-1) for x in ts])
        p += t.numel()
    if len(ts) == 1:
        return ts[0].reshape(-1)
    return torch.as_strided(ts[0], (p - ts[0].data_ptr(),), (1,))


def _ragged_images(ims, rgb_offs=None):
    """the lrf_ragged_image array of a checked image list (check_ragged_args); rgb_offs: where each image's output starts, else 0"""
    desc = (RaggedImage * len(ims))()
    for i, (d, (H, W, ranks, u_off, v_off)) in enumerate(zip(desc, ims)):
        d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, u_off, v_off, 0 if rgb_offs is None else rgb_offs[i]
        d.R[0], d.R[1], d.R[2] = ranks
    return desc


def _packed_outputs(sizes, channels=3):
    """[channels, h, w] outputs in one buffer, each starting at a multiple of 16 bytes -> (their offsets, the buffer's size)"""
    offs, off = [], 0
    for h, w in sizes:
        offs.append(off)
        off = (off + channels * h * w + 15) // 16 * 16
    return offs, off


def _dptr(t):
    """device pointer of a torch CUDA tensor (must be contiguous) or None"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous CUDA tensor"
    return c_void_p(t.data_ptr())


class Context:
    """One lrf_ctx: a device, a stream and the scratch workspace.  Not thread-safe."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = c_void_p()
        check(self._lib.lrf_ctx_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)

    def close(self):
        if self._h:
            self._lib.lrf_ctx_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self):
        import torch
        check(self._lib.lrf_ctx_set_stream(self._h, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _need_here(self, entry, t):
        if not (t.is_cuda and t.device.index == self.device):
            raise ValueError(f"{entry} needs its tensors on cuda:{self.device}, got {t.device}")

    def synchronize(self):
        check(self._lib.lrf_ctx_synchronize(self._h))

    def check(self):
        """Raises LrfError if a persistent launch (k_bcd_p) on this context gave up since the last look (include/lrf_hip.h,
        lrf_ctx_check).  Does not wait: call it once the stream has been waited for — after `.cpu()` of a result, a
        torch.cuda.synchronize().  Every wrapper that hands results to the host calls it (`to_host`)."""
        check(self._lib.lrf_ctx_check(self._h))

    def last_luma_source(self):
        """"bytes" when the persistent kernel of this context's last encode_rgb read the luma matrices from the image bytes,
        "x" when from the fp32 workspace, None before the first such call (lrf_ctx_last_luma_source; the factors are the same
        bit for bit)"""
        return {0: "x", 1: "bytes"}.get(int(self._lib.lrf_ctx_last_luma_source(self._h)))

    def last_x_residency(self):
        """(kept planes, kept bytes) of this context's last encode_rgb: the chroma planes whose X the persistent kernel loads on
        the default cache policy, so that they stay in the Infinity Cache from one iteration to the next, while the rest of the
        call streams non-temporal; (0, 0) when the policy did not apply, None before the first such call
        (lrf_ctx_last_x_residency; the factors are the same bit for bit)"""
        nbytes = c_i64(-1)
        planes = int(self._lib.lrf_ctx_last_x_residency(self._h, ctypes.byref(nbytes)))
        return None if planes < 0 else (planes, int(nbytes.value))

    def to_host(self, *tensors):
        """the tensors on the host (torch's copy waits for the stream the kernels ran on), then `check`: the one way results
        of the encoder leave the device in this package, so that a failed launch raises in the call it belongs to"""
        out = tuple(t.cpu() for t in tensors)
        self.check()
        return out

    def workspace_bytes(self):
        return int(self._lib.lrf_ctx_workspace_bytes(self._h))

    def trim(self):
        """waits for the stream and releases the scratch workspace (it is re-grown by the next call)"""
        check(self._lib.lrf_ctx_trim(self._h))

    def profile(self, enable=True):
        check(self._lib.lrf_ctx_profile(self._h, int(bool(enable))))

    def profile_kernels(self, kernel_ids):
        """event-time only these kernel ids (an iterable of LRF_K_* numbers; empty = off)"""
        mask = 0
        for k in kernel_ids:
            mask |= 1 << int(k)
        check(self._lib.lrf_ctx_profile_kernels(self._h, mask))

    def profile_reset(self):
        check(self._lib.lrf_ctx_profile_reset(self._h))

    def kernel_time(self, kernel_id):
        ms, n = ctypes.c_double(), ctypes.c_long()
        check(self._lib.lrf_ctx_kernel_time(self._h, kernel_id, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    # ---- hot path (torch CUDA tensors in / out) ----
    def planes_from_rgb(self, rgb):
        import torch
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        floats = sum(d[4] for d in plane_dims(H, W)) * 64
        X = torch.empty((B, floats), dtype=torch.float32, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_planes_from_rgb_u8(self._h, _dptr(rgb), B, H, W, _dptr(X)))
        return X

    def decompose(self, X, R, K, lo, hi, sign=None):
        import torch
        X = X.contiguous()
        B, M, N = X.shape
        U = torch.empty((B, M, R), dtype=torch.int8, device=X.device)
        V = torch.empty((B, N, R), dtype=torch.int8, device=X.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decompose_f32(self._h, _dptr(X), B, M, N, R, K, lo, hi, _dptr(sign), _dptr(U), _dptr(V)))
        return U, V

    def decompose_ex(self, X, R, K, bounds=(None, None), l2=0.0, l1_ratio=0.0, factor=(0, 1, 2), sign=None, init=None, eps=1e-16, w_init=None):
        """The general QMF.decompose (lrf_qmf_decompose_ex_f32): X [B,M,N] fp32 CUDA -> fp32 (U [B,M,R], V [B,N,R], W [B,2]).
        init = (u0, v0): initial factors instead of the library's SVD; w_init [B,2]: the initial affine pair that belongs to
        them (SVDInit(num_levels=...)); eps: CoordinateDescent's eps."""
        import torch
        X = X.float().contiguous()
        B, M, N = X.shape
        U = torch.empty((B, M, R), dtype=torch.float32, device=X.device)
        V = torch.empty((B, N, R), dtype=torch.float32, device=X.device)
        W = torch.empty((B, 2), dtype=torch.float32, device=X.device)
        bounded = bounds is not None and tuple(bounds) != (None, None)
        l2 = tuple(l2) if isinstance(l2, (tuple, list)) else (l2, l2)
        opts = QmfOpts(int(bounded), float(bounds[0]) if bounded else 0.0, float(bounds[1]) if bounded else 0.0, float(l2[0]), float(l2[1]),
                       float(l1_ratio), sum(1 << int(f) for f in set(factor)), 0.0 if eps == 1e-16 else float(eps), int(w_init is not None))
        if w_init is not None:
            assert init is not None, "w_init belongs to initial factors"
            W.copy_(w_init.to(device=X.device, dtype=torch.float32).reshape(B, 2))
        u0 = v0 = None
        if init is not None:
            u0, v0 = (t.to(device=X.device, dtype=torch.float32).contiguous() for t in init)
            assert tuple(u0.shape) == (B, M, R) and tuple(v0.shape) == (B, N, R)
        if sign is not None:
            sign = sign.to(device=X.device, dtype=torch.int8).contiguous()
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decompose_ex_f32(self._h, _dptr(X), B, M, N, int(R), int(K), ctypes.byref(opts), _dptr(sign), _dptr(u0),
                                                 _dptr(v0), _dptr(U), _dptr(V), _dptr(W)))
        return U, V, W

    def bcd(self, X, U0, V0, K, lo, hi):
        import torch
        X, U0, V0 = X.contiguous(), U0.float().contiguous(), V0.float().contiguous()
        B, M, N = X.shape
        R = U0.shape[-1]
        U = torch.empty((B, M, R), dtype=torch.int8, device=X.device)
        V = torch.empty((B, N, R), dtype=torch.int8, device=X.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_bcd_f32(self._h, _dptr(X), B, M, N, R, K, lo, hi, _dptr(U0), _dptr(V0), _dptr(U), _dptr(V)))
        return U, V

    def svd_init(self, X, R, sign=None):
        import torch
        X = X.contiguous()
        B, M, N = X.shape
        U0 = torch.empty((B, M, R), dtype=torch.float32, device=X.device)
        V0 = torch.empty((B, N, R), dtype=torch.float32, device=X.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_svd_init_f32(self._h, _dptr(X), B, M, N, R, _dptr(sign), _dptr(U0), _dptr(V0)))
        return U0, V0

    def loss(self, X, U, V, W=None):
        """QMF.loss per matrix (lrf_qmf_loss_f32): X [B,M,N], U [B,M,R], V [B,N,R] fp32 CUDA, W [B,2] or None -> fp32 [B]"""
        import torch
        X, U, V = X.float().contiguous(), U.float().contiguous(), V.float().contiguous()
        B, M, N = X.shape
        R = U.shape[-1]
        assert tuple(U.shape) == (B, M, R) and tuple(V.shape) == (B, N, R)
        if W is not None:
            W = W.to(device=X.device, dtype=torch.float32).reshape(B, 2).contiguous()
        out = torch.empty((B,), dtype=torch.float32, device=X.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_loss_f32(self._h, _dptr(X), _dptr(U), _dptr(V), _dptr(W), B, M, N, int(R), _dptr(out)))
        return out

    def encode_rgb(self, rgb, ranks, K, lo, hi, sign=None, out=None):
        """rgb uint8 [B,3,H,W] (CUDA) -> (U int8 [B, sum M_c R_c], V int8 [B, 64 sum R_c])"""
        import torch
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        dims = plane_dims(H, W)
        nu = sum(d[4] * r for d, r in zip(dims, ranks))
        nv = 64 * sum(ranks)
        if out is None:
            U = torch.empty((B, nu), dtype=torch.int8, device=rgb.device)
            V = torch.empty((B, nv), dtype=torch.int8, device=rgb.device)
        else:  # the kernels write B * nu / B * nv bytes: anything else would be an out-of-bounds device write
            U, V = out
            for t, n, name in ((U, nu, "U"), (V, nv, "V")):
                if not (t.is_cuda and t.device == rgb.device and t.dtype == torch.int8 and t.is_contiguous()
                        and tuple(t.shape) == (B, n)):
                    raise ValueError(f"out {name} must be a contiguous int8 tensor of shape {(B, n)} on {rgb.device}")
        R = (c_int * 3)(*[int(r) for r in ranks])
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_rgb_u8(self._h, _dptr(rgb), B, H, W, R, K, lo, hi, _dptr(sign), _dptr(U), _dptr(V)))
        return U, V

    def encode_sweep_rgb(self, rgb, triples, K, lo, hi, sign=None):
        """rgb uint8 [B,3,H,W] (CUDA) at every rank triple of `triples` in ONE call (lrf_qmf_encode_sweep_rgb_u8) ->
        [(U int8 [B, sum M_c R_c], V int8 [B, 64 sum R_c]) per triple] (views of two flat buffers)"""
        import torch
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8 and len(triples) >= 1
        dims = plane_dims(H, W)
        nus = [sum(d[4] * int(r) for d, r in zip(dims, t)) for t in triples]
        nvs = [64 * sum(int(r) for r in t) for t in triples]
        U = torch.empty((B * sum(nus),), dtype=torch.int8, device=rgb.device)
        V = torch.empty((B * sum(nvs),), dtype=torch.int8, device=rgb.device)
        R = (c_int * (3 * len(triples)))(*[int(r) for t in triples for r in t])
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_sweep_rgb_u8(self._h, _dptr(rgb), B, H, W, len(triples), R, K, lo, hi, _dptr(sign), _dptr(U), _dptr(V)))
        out, uo, vo = [], 0, 0
        for nu, nv in zip(nus, nvs):
            out.append((U[uo:uo + B * nu].view(B, nu), V[vo:vo + B * nv].view(B, nv)))
            uo += B * nu
            vo += B * nv
        return out

    def decode_rgb(self, U, V, H, W, ranks):
        import torch
        U, V = U.contiguous(), V.contiguous()
        B = U.shape[0]
        # the kernel indexes the factors from (H, W) and the ranks alone: sizes that disagree would be out-of-bounds reads
        dims = plane_dims(H, W)
        nu, nv = sum(d[4] * int(r) for d, r in zip(dims, ranks)), 64 * sum(int(r) for r in ranks)
        if len(ranks) != 3 or U.dtype != torch.int8 or V.dtype != torch.int8 or tuple(U.shape) != (B, nu) or \
                tuple(V.shape) != (B, nv) or V.device != U.device:
            raise ValueError(f"factor buffers do not match the geometry: expected int8 U {(B, nu)} and V {(B, nv)}, "
                             f"got {U.dtype} {tuple(U.shape)} and {V.dtype} {tuple(V.shape)}")
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=U.device)
        R = (c_int * 3)(*[int(r) for r in ranks])
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_rgb_u8(self._h, _dptr(U), _dptr(V), B, H, W, R, _dptr(rgb)))
        return rgb

    def decode_ragged(self, U, V, images):
        """Images that differ in size and ranks in one call (lrf_qmf_decode_ragged_rgb_u8).  U, V: flat int8 CUDA tensors; images:
        [(H, W, ranks, u_off, v_off)], image i's factors at U[u_off:], V[v_off:] in encode_rgb's layout of one image -> a list
        of uint8 CUDA tensors [3,H_i,W_i]: views of one buffer, each starting at a multiple of 16 bytes (so that images whose
        sides are multiples of 16 keep the decoder made for them)."""
        import torch
        ims = check_ragged_args(U, V, images)
        self._need_here("decode_ragged", U)
        offs, total = _packed_outputs([im[:2] for im in ims])
        desc = _ragged_images(ims, offs)
        rgb = torch.empty((total,), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_ragged_rgb_u8(self._h, len(ims), desc, _dptr(U), U.numel(), _dptr(V), V.numel(), _dptr(rgb), rgb.numel()))
        return [rgb[d.rgb_off:d.rgb_off + 3 * d.H * d.W].view(3, d.H, d.W) for d in desc]

    def _decode_windows(self, method, U, V, desc, boxes, crop_type, size, fmt, tensor):
        """The ctypes call of one of the ten C entries that decode crops, every argument checked by the caller.  method: the public
        method's name, which names the rest: the C entries are lrf_qmf_<method>_rgb_u8 (gray: _u8) for fmt None and
        lrf_qmf_<method>_tensor for a TensorFormat, and output refusals carry the name without "gray_".  desc: the lrf_ragged_image
        or lrf_gray_image array (which says how many channels); boxes: int32 rows of crop_type; size: (h, w) or (oh, ow); tensor:
        the caller's (dtype, channels_last, out) -> [n, channels, h, w], `out` if given."""
        import torch
        channels = 1 if desc._type_ is GrayImage else 3
        dtype, channels_last, out = tensor
        self._need_here(method, U)
        n, (h, w) = boxes.shape[0], size
        lead = (self._h, len(desc), desc, _dptr(U), U.numel(), _dptr(V), V.numel(), n, boxes.ctypes.data_as(ctypes.POINTER(crop_type)), h, w)
        if fmt is not None:
            res = _tensor_output(method.replace("gray_", ""), out, n, h, w, dtype, channels_last, U.device, channels)
            self.use_torch_stream()
            check(getattr(self._lib, f"lrf_qmf_{method}_tensor")(*lead, ctypes.byref(fmt), c_void_p(res.data_ptr()), res.numel() * res.element_size()))
            return res
        res = torch.empty((n, channels, h, w), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(getattr(self._lib, f"lrf_qmf_{method}_{'rgb_u8' if channels == 3 else 'u8'}")(*lead, _dptr(res), res.numel()))
        return res

    def decode_crops(self, U, V, images, crops, size, dtype=None, mean=None, std=None, channels_last=False, out=None):
        """Windows straight from the factors (lrf_qmf_decode_crops_rgb_u8).  U, V, images: as decode_ragged takes them; crops: an
        integer array-like [n, 3] of (image, y0, x0) on the host; size: (h, w) -> a uint8 CUDA tensor [n, 3, h, w], crop j equal
        to the decode of its image sliced [:, y0:y0+h, x0:x0+w].  Asynchronous on torch's current stream; a new crop list costs no
        stream wait (a new image list does, once).
        dtype=torch.float32 / float16 / bfloat16 (default torch.uint8: the above): the model's tensor instead
        (lrf_qmf_decode_crops_tensor), logical shape [n, 3, h, w], every byte b of the above as (b * scale_k) + bias_k in fp32 (two
        roundings) rounded to dtype; mean, std: as check_tensor_format takes them; channels_last: torch.channels_last memory;
        out: a tensor of that dtype, shape, device and memory format (a slice along n of a larger batch, say), written in place."""
        import torch
        fmt = _tensor_request("decode_crops", torch.uint8 if dtype is None else dtype, mean, std, channels_last, out)
        ims, boxes, size = check_crop_args(U, V, images, crops, size)
        return self._decode_windows("decode_crops", U, V, desc=_ragged_images(ims), boxes=boxes, crop_type=Crop, size=size, fmt=fmt,
                                    tensor=(dtype, channels_last, out))

    def decode_scaled(self, U, V, images, scale):
        """Images at 1/scale straight from the factors (lrf_qmf_decode_scaled_rgb_u8).  U, V, images: as decode_ragged takes them;
        scale: 2, 4 or 8 -> a list of uint8 CUDA tensors [3, ceil(H_i / scale), ceil(W_i / scale)]: views of one buffer, each
        starting at a multiple of 16 bytes.  Asynchronous on torch's current stream."""
        import torch
        ims, scale = check_scaled_args(U, V, images, scale)
        self._need_here("decode_scaled", U)
        sizes = [scaled_dims(H, W, scale) for H, W, *_ in ims]
        offs, total = _packed_outputs(sizes)
        desc = _ragged_images(ims, offs)
        rgb = torch.empty((total,), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_scaled_rgb_u8(self._h, len(ims), desc, scale, _dptr(U), U.numel(), _dptr(V), V.numel(), _dptr(rgb), rgb.numel()))
        return [rgb[d.rgb_off:d.rgb_off + 3 * hs * ws].view(3, hs, ws) for d, (hs, ws) in zip(desc, sizes)]

    def decode_scaled_crops(self, U, V, images, crops, size, dtype=None, mean=None, std=None, channels_last=False, out=None):
        """Windows of scaled images straight from the factors (lrf_qmf_decode_scaled_crops_rgb_u8).  U, V, images: as decode_ragged
        takes them; crops: an integer array-like [n, 4] of (image, scale, y0, x0) on the host, the scale per crop out of 2, 4, 8
        and y0, x0 in the scaled image; size: (h, w) -> a uint8 CUDA tensor [n, 3, h, w], crop j equal to decode_scaled of its
        image at its scale sliced [:, y0:y0+h, x0:x0+w].  Asynchronous on torch's current stream.
        dtype, mean, std, channels_last, out: as decode_crops takes them (lrf_qmf_decode_scaled_crops_tensor)."""
        import torch
        fmt = _tensor_request("decode_scaled_crops", torch.uint8 if dtype is None else dtype, mean, std, channels_last, out)
        ims, boxes, size = check_scaled_args(U, V, images, crops=crops, size=size)
        return self._decode_windows("decode_scaled_crops", U, V, desc=_ragged_images(ims), boxes=boxes, crop_type=ScaledCrop, size=size, fmt=fmt,
                                    tensor=(dtype, channels_last, out))

    def decode_resized_crops(self, U, V, images, crops, size, dtype=None, mean=None, std=None, channels_last=False, out=None):
        """Boxes of any size resampled to one output size straight from the factors (lrf_qmf_decode_resized_crops_rgb_u8).  U, V,
        images: as decode_ragged takes them; crops: an integer array-like [n, 6] of (image, y0, x0, h, w, flip) on the host, the
        box in full-resolution pixels; size: (oh, ow) -> a uint8 CUDA tensor [n, 3, oh, ow].  Crop j is the fixed-point bilinear
        resampling include/lrf_hip.h defines, from the level (1, 1/2, 1/4, 1/8) nearest above the output's size: not torchvision's
        bytes.  Asynchronous on torch's current stream; a new crop list costs no stream wait.
        dtype, mean, std, channels_last, out: as decode_crops takes them (lrf_qmf_decode_resized_crops_tensor): resized crop, flip,
        to-tensor and normalise in one call, no uint8 batch in between."""
        import torch
        fmt = _tensor_request("decode_resized_crops", torch.uint8 if dtype is None else dtype, mean, std, channels_last, out)
        ims, boxes, size = check_resized_args(U, V, images, crops, size)
        return self._decode_windows("decode_resized_crops", U, V, desc=_ragged_images(ims), boxes=boxes, crop_type=ResizedCrop, size=size, fmt=fmt,
                                    tensor=(dtype, channels_last, out))

    def decode_gray_ragged(self, U, V, images, scale=1):
        """Gray images that differ in size and rank in one call, whole or at 1/2, 1/4, 1/8 scale (lrf_qmf_decode_gray_ragged_u8).
        U, V: flat int8 CUDA tensors; images: [(H, W, R, u_off, v_off)], image i's U [M, R] at U[u_off:], V [64, R] at V[v_off:];
        scale: 1, 2, 4 or 8 -> a list of uint8 CUDA tensors [1, ceil(H_i / scale), ceil(W_i / scale)]: views of one buffer, each
        starting at a multiple of 16 bytes.  Asynchronous on torch's current stream."""
        import torch
        ims, scale = check_gray_images(U, V, images), check_gray_scale(scale)
        self._need_here("decode_gray_ragged", U)
        sizes = [gray_scaled_dims(H, W, scale) for H, W, *_ in ims]
        offs, off = _packed_outputs(sizes, channels=1)
        desc = _gray_images(ims, offs)
        out = torch.empty((off,), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_gray_ragged_u8(self._h, len(ims), desc, scale, _dptr(U), U.numel(), _dptr(V), V.numel(), _dptr(out), out.numel()))
        return [out[o:o + hs * ws].view(1, hs, ws) for o, (hs, ws) in zip(offs, sizes)]

    def decode_gray_crops(self, U, V, images, crops, size, dtype=None, mean=None, std=None, channels_last=False, out=None):
        """Windows of gray images straight from the factors, each at its own level (lrf_qmf_decode_gray_crops_u8).  U, V, images: as
        decode_gray_ragged takes them; crops: an integer array-like [n, 4] of (image, scale, y0, x0) on the host, the scale per
        crop out of 1, 2, 4, 8 and y0, x0 in the image at that scale; size: (h, w) -> a uint8 CUDA tensor [n, 1, h, w], crop j equal
        to decode_gray_ragged of its image at its scale sliced [:, y0:y0+h, x0:x0+w].  Asynchronous on torch's current stream; a new
        crop list costs no stream wait (a new image list does, once).
        dtype=torch.float32 / float16 / bfloat16: the model's tensor instead (lrf_qmf_decode_gray_crops_tensor), every byte b as
        (b * scale) + bias in fp32 (two roundings) rounded to dtype; mean, std: None, one number or a sequence of one;
        channels_last: validated and otherwise immaterial (one channel: the same memory); out: a dense [n, 1, h, w] tensor of that
        dtype on this device (a slice along n of a larger batch, say), written in place."""
        import torch
        fmt = check_gray_tensor_request("decode_crops", torch.uint8 if dtype is None else dtype, mean, std, channels_last, out)
        ims, boxes, size = check_gray_crop_args(U, V, images, crops, size)
        return self._decode_windows("decode_gray_crops", U, V, desc=_gray_images(ims), boxes=boxes, crop_type=ScaledCrop, size=size, fmt=fmt,
                                    tensor=(dtype, channels_last, out))

    def decode_gray_resized_crops(self, U, V, images, crops, size, dtype=None, mean=None, std=None, channels_last=False, out=None):
        """Boxes of any size out of gray images resampled to one output size straight from the factors
        (lrf_qmf_decode_gray_resized_crops_u8).  U, V, images: as decode_gray_ragged takes them; crops: an integer array-like
        [n, 6] of (image, y0, x0, h, w, flip) on the host, the box in full-resolution pixels; size: (oh, ow) -> a uint8 CUDA
        tensor [n, 1, oh, ow]: the level rule, taps and blend of decode_resized_crops on the gray levels.
        dtype, mean, std, channels_last, out: as decode_gray_crops takes them (lrf_qmf_decode_gray_resized_crops_tensor)."""
        import torch
        fmt = check_gray_tensor_request("decode_resized_crops", torch.uint8 if dtype is None else dtype, mean, std, channels_last, out)
        ims, boxes, size = check_gray_resized_args(U, V, images, crops, size)
        return self._decode_windows("decode_gray_resized_crops", U, V, desc=_gray_images(ims), boxes=boxes, crop_type=ResizedCrop, size=size, fmt=fmt,
                                    tensor=(dtype, channels_last, out))

    def encode_ragged(self, rgb, images, K, lo, hi, sign=None):
        """Images that differ in size and ranks in one encode (lrf_qmf_encode_ragged_rgb_u8).  rgb: a flat uint8 CUDA tensor;
        images: [(H, W, ranks, rgb_off[, sign_off])], image i's [3,H,W] bytes at rgb[rgb_off:]; sign: None or a flat int8 CUDA
        tensor -> (U, V, u_off, v_off): two flat int8 CUDA tensors and, per image, where its factors start in them, each image
        in encode_rgb's layout of one image, the images back to back in call order."""
        import torch
        ims = check_encode_ragged_args(rgb, images, sign)
        self._need_here("encode_ragged", rgb)
        desc = (RaggedEncodeImage * len(ims))()
        u_off, v_off, uo, vo = [], [], 0, 0
        for d, (H, W, ranks, rgb_off, sign_off) in zip(desc, ims):
            d.H, d.W, d.rgb_off, d.u_off, d.v_off, d.sign_off = H, W, rgb_off, uo, vo, sign_off
            d.R[0], d.R[1], d.R[2] = ranks
            u_off.append(uo)
            v_off.append(vo)
            uo += sum(dm[4] * r for dm, r in zip(plane_dims(H, W), ranks))
            vo += 64 * sum(ranks)
        U = torch.empty((uo,), dtype=torch.int8, device=rgb.device)
        V = torch.empty((vo,), dtype=torch.int8, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_ragged_rgb_u8(self._h, len(ims), desc, _dptr(rgb), rgb.numel(), int(K), int(lo), int(hi), _dptr(sign),
                                                     0 if sign is None else sign.numel(), _dptr(U), uo, _dptr(V), vo))
        return U, V, u_off, v_off

    def encode_ragged_sweep(self, rgb, images, cands, K, lo, hi, sign=None):
        """Images that differ in size, each at candidate rank triples of its own, in one encode
        (lrf_qmf_encode_ragged_sweep_rgb_u8).  rgb: a flat uint8 CUDA tensor; images: [(H, W, rgb_off[, sign_off])]; cands:
        [(image, ranks)] in any order, at least one per image; sign: None or a flat int8 CUDA tensor holding, per image with a
        sign_off, the signs of its largest rank per channel -> (U, V, u_off, v_off): two flat int8 CUDA tensors and, per
        candidate, where its factors start in them, each in encode_rgb's layout of one image, back to back in list order."""
        import torch
        ims, cd = _check_encode_ragged_sweep(rgb, images, cands, sign)
        self._need_here("encode_ragged_sweep", rgb)
        idesc = (RaggedSweepImage * len(ims))()
        for d, (H, W, rgb_off, sign_off) in zip(idesc, ims):
            d.H, d.W, d.rgb_off, d.sign_off = H, W, rgb_off, sign_off
        ims_a = np.array(ims, dtype=np.int64).reshape(-1, 4)
        Ms = plane_patches(ims_a[:, 0], ims_a[:, 1])[cd[:, 0]]
        nu, nv = (Ms * cd[:, 1:]).sum(axis=1), 64 * cd[:, 1:].sum(axis=1)
        assert _SWEEP_CAND_DT.itemsize == ctypes.sizeof(RaggedSweepCandidate)
        rec = np.zeros((cd.shape[0],), dtype=_SWEEP_CAND_DT)
        rec["image"], rec["R"], rec["u_off"], rec["v_off"] = cd[:, 0], cd[:, 1:], np.cumsum(nu) - nu, np.cumsum(nv) - nv
        cdesc = rec.ctypes.data_as(ctypes.POINTER(RaggedSweepCandidate))
        u_off, v_off, uo, vo = rec["u_off"].tolist(), rec["v_off"].tolist(), int(nu.sum()), int(nv.sum())
        U = torch.empty((uo,), dtype=torch.int8, device=rgb.device)
        V = torch.empty((vo,), dtype=torch.int8, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_ragged_sweep_rgb_u8(self._h, len(ims), idesc, int(cd.shape[0]), cdesc, _dptr(rgb), rgb.numel(), int(K), int(lo), int(hi),
                                                           _dptr(sign), 0 if sign is None else sign.numel(), _dptr(U), uo, _dptr(V), vo))
        return U, V, u_off, v_off

    def sse_ragged(self, rgb, items, U, V):
        """The squared error of items that differ in size and ranks straight from their factors (lrf_qmf_sse_ragged_rgb_u8).  rgb:
        a flat uint8 CUDA tensor holding the sources; items: [(H, W, ranks, u_off, v_off, rgb_off)] (or an integer array [n, 8] with
        the ranks spread out), item i's factors at
        U[u_off:], V[v_off:] and its source [3,H,W] at rgb[rgb_off:] (several items may share a source) -> int64 CUDA tensor
        [len(items)], sse[i] = ((decode_ragged's image of item i).long() - source.long()) ** 2 summed, without the decoded
        images.  Lists above 65535 items take one call per 65535.  Asynchronous on torch's current stream."""
        import torch
        its = _sse_items_array(rgb, items, U, V)
        self._need_here("sse_ragged", rgb)
        assert _RAGGED_IMAGE_DT.itemsize == ctypes.sizeof(RaggedImage)
        rec = np.zeros((its.shape[0],), dtype=_RAGGED_IMAGE_DT)
        rec["H"], rec["W"], rec["R"], rec["u_off"], rec["v_off"], rec["rgb_off"] = its[:, 0], its[:, 1], its[:, 2:5], its[:, 5], its[:, 6], its[:, 7]
        sse = torch.empty((its.shape[0],), dtype=torch.int64, device=rgb.device)
        self.use_torch_stream()
        for k in range(0, its.shape[0], 65535):
            part = rec[k:k + 65535]
            check(self._lib.lrf_qmf_sse_ragged_rgb_u8(self._h, part.shape[0], part.ctypes.data_as(ctypes.POINTER(RaggedImage)), _dptr(U), U.numel(), _dptr(V),
                                                      V.numel(), _dptr(rgb), rgb.numel(), c_void_p(sse[k:].data_ptr())))
        return sse

    def ssim_ragged(self, rgb, items, U, V, scratch_bytes=0):
        """The squared error and the SSIM of items that differ in size and ranks, scored from their factors
        (lrf_qmf_ssim_ragged_rgb_u8): sse_ragged's arguments -> (sse int64 [n], ssim float64 [n]) on the device, what decode_ragged
        followed by image_metrics(source[None], decoded[None]) gives per item, bit for bit.  The decoded images live chunk by
        chunk in the context's scratch buffer of at most scratch_bytes (0: 256 MiB; an item larger than the cap is a chunk of
        its own); the results do not depend on it.  Lists above 65535 items take one call per 65535.  Asynchronous on torch's
        current stream."""
        import torch
        its = check_ssim_ragged_args(rgb, items, U, V, scratch_bytes)
        self._need_here("ssim_ragged", rgb)
        assert _RAGGED_IMAGE_DT.itemsize == ctypes.sizeof(RaggedImage)
        rec = np.zeros((its.shape[0],), dtype=_RAGGED_IMAGE_DT)
        rec["H"], rec["W"], rec["R"], rec["u_off"], rec["v_off"], rec["rgb_off"] = its[:, 0], its[:, 1], its[:, 2:5], its[:, 5], its[:, 6], its[:, 7]
        sse = torch.empty((its.shape[0],), dtype=torch.int64, device=rgb.device)
        ssim = torch.empty((its.shape[0],), dtype=torch.float64, device=rgb.device)
        self.use_torch_stream()
        for k in range(0, its.shape[0], 65535):
            part = rec[k:k + 65535]
            check(self._lib.lrf_qmf_ssim_ragged_rgb_u8(self._h, part.shape[0], part.ctypes.data_as(ctypes.POINTER(RaggedImage)), _dptr(U), U.numel(), _dptr(V),
                                                       V.numel(), _dptr(rgb), rgb.numel(), int(scratch_bytes), c_void_p(sse[k:].data_ptr()),
                                                       c_void_p(ssim[k:].data_ptr())))
        return sse, ssim

    def metrics_ragged(self, a, b, pairs, C, want_ssim=True):
        """The squared error and the SSIM of pairs that differ in size (lrf_image_metrics_ragged_u8).  a, b: flat uint8 CUDA
        tensors; pairs: [(H, W, a_off, b_off)] (or an integer array [n, 4]), pair i's images [C,H,W] at a[a_off:] and b[b_off:]
        (several pairs may share an a image) -> (sse int64 [n], ssim float64 [n] or None) on the device, per pair what
        image_metrics gives for that pair alone, bit for bit.  Asynchronous on torch's current stream."""
        import torch
        for t in (a, b):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise TypeError("metrics_ragged takes its images as uint8 tensors")
            if t.dim() != 1 or not t.is_contiguous():
                raise ValueError("metrics_ragged takes its images as flat contiguous tensors")
        if a.device != b.device:
            raise ValueError(f"metrics_ragged needs its tensors on one device, got {a.device} and {b.device}")
        raw = np.asarray(pairs)
        if raw.ndim != 2 or raw.shape[1] != 4 or raw.shape[0] < 1 or raw.shape[0] > 65535 or raw.dtype.kind not in "iu":
            raise ValueError("metrics_ragged takes 1 to 65535 pairs of integers (H, W, a_off, b_off)")
        p = np.ascontiguousarray(raw.astype(np.int64))
        C = int(C)
        if C < 1 or C > 65535:
            raise ValueError(f"C={C} out of range [1,65535]")
        lo = 7 if want_ssim else 1
        bad = (p[:, :2].min(axis=1) < lo) | (p[:, :2].max(axis=1) > 2 ** 20)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"pair {i}: size {p[i, 0]}x{p[i, 1]} out of range" + (" (win_size exceeds image extent.)" if p[i, :2].min() < 7 else ""))
        px = C * p[:, 0] * p[:, 1]
        bad = (p[:, 2] < 0) | (p[:, 3] < 0) | (p[:, 2] > a.numel() - px) | (p[:, 3] > b.numel() - px)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"pair {i}: its images of {px[i]} bytes at {p[i, 2]} and {p[i, 3]} leave the buffers of {a.numel()} and {b.numel()} bytes")
        self._need_here("metrics_ragged", a)
        sse = torch.empty((p.shape[0],), dtype=torch.int64, device=a.device)
        ssim = torch.empty((p.shape[0],), dtype=torch.float64, device=a.device) if want_ssim else None
        self.use_torch_stream()
        check(self._lib.lrf_image_metrics_ragged_u8(self._h, p.shape[0], c_void_p(p.ctypes.data), C, _dptr(a), a.numel(), _dptr(b), b.numel(), _dptr(sse),
                                                    _dptr(ssim)))
        return sse, ssim

    def encode_gray_ragged(self, gray, images, K, lo, hi, sign=None):
        """Gray images that differ in size and rank in one encode (lrf_qmf_encode_gray_ragged_u8).  gray: a flat uint8 CUDA tensor;
        images: [(H, W, R, gray_off[, sign_off])], image i's [H, W] bytes at gray[gray_off:]; sign: None or a flat int8 CUDA tensor
        -> (U, V, u_off, v_off): two flat int8 CUDA tensors and, per image, where its U [M, R] and V [64, R] start in them, back
        to back in call order: the bytes of encode_gray on that image alone.  Asynchronous on torch's current stream."""
        import torch
        ims = check_encode_gray_ragged_args(gray, images, sign)
        self._need_here("encode_gray_ragged", gray)
        desc = (GrayEncodeImage * len(ims))()
        u_off, v_off, uo, vo = [], [], 0, 0
        for d, (H, W, R, gray_off, sign_off) in zip(desc, ims):
            d.H, d.W, d.R, d.gray_off, d.u_off, d.v_off, d.sign_off = H, W, R, gray_off, uo, vo, sign_off
            u_off.append(uo)
            v_off.append(vo)
            uo += chan_dims(H, W, 1, (8, 8))[2] * R
            vo += 64 * R
        U = torch.empty((uo,), dtype=torch.int8, device=gray.device)
        V = torch.empty((vo,), dtype=torch.int8, device=gray.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_gray_ragged_u8(self._h, len(ims), desc, _dptr(gray), gray.numel(), int(K), int(lo), int(hi), _dptr(sign),
                                                      0 if sign is None else sign.numel(), _dptr(U), uo, _dptr(V), vo))
        return U, V, u_off, v_off

    def encode_gray_ragged_sweep(self, gray, images, cands, K, lo, hi, sign=None):
        """Gray images that differ in size, each at candidate ranks of its own, in one encode
        (lrf_qmf_encode_gray_ragged_sweep_u8).  gray: a flat uint8 CUDA tensor; images: [(H, W, gray_off[, sign_off])]; cands:
        [(image, R)] in any order, at least one per image; sign: None or a flat int8 CUDA tensor holding, per image with a
        sign_off, the signs of its largest rank -> (U, V, u_off, v_off): two flat int8 CUDA tensors and, per candidate, where its
        U [M, R] and V [64, R] start in them, back to back in list order: the bytes of encode_gray_ragged for (image, R) alone."""
        import torch
        ims, cds = check_encode_gray_ragged_sweep_args(gray, images, cands, sign)
        self._need_here("encode_gray_ragged_sweep", gray)
        idesc = (GraySweepImage * len(ims))()
        for d, (H, W, gray_off, sign_off) in zip(idesc, ims):
            d.H, d.W, d.gray_off, d.sign_off = H, W, gray_off, sign_off
        Ms = [chan_dims(H, W, 1, (8, 8))[2] for H, W, *_ in ims]
        cdesc = (GraySweepCandidate * len(cds))()
        u_off, v_off, uo, vo = [], [], 0, 0
        for d, (image, R) in zip(cdesc, cds):
            d.image, d.R, d.u_off, d.v_off = image, R, uo, vo
            u_off.append(uo)
            v_off.append(vo)
            uo += Ms[image] * R
            vo += 64 * R
        U = torch.empty((uo,), dtype=torch.int8, device=gray.device)
        V = torch.empty((vo,), dtype=torch.int8, device=gray.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_gray_ragged_sweep_u8(self._h, len(ims), idesc, len(cds), cdesc, _dptr(gray), gray.numel(), int(K), int(lo), int(hi),
                                                            _dptr(sign), 0 if sign is None else sign.numel(), _dptr(U), uo, _dptr(V), vo))
        return U, V, u_off, v_off

    def sse_gray_ragged(self, gray, items, U, V):
        """The squared error of gray items that differ in size and rank straight from their factors (lrf_qmf_sse_gray_ragged_u8).
        gray: a flat uint8 CUDA tensor holding the sources; items: [(H, W, R, u_off, v_off, gray_off)], item i's factors at
        U[u_off:], V[v_off:] and its source [H, W] at gray[gray_off:] (several items may share a source) -> int64 CUDA tensor
        [len(items)], sse[i] = ((decode_gray_ragged's image of item i).long() - source.long()) ** 2 summed, without the decoded
        images.  Asynchronous on torch's current stream."""
        import torch
        its = check_sse_gray_ragged_args(gray, items, U, V)
        self._need_here("sse_gray_ragged", gray)
        desc = _gray_images([it[:5] for it in its], [it[5] for it in its])
        sse = torch.empty((len(its),), dtype=torch.int64, device=gray.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_sse_gray_ragged_u8(self._h, len(its), desc, _dptr(U), U.numel(), _dptr(V), V.numel(), _dptr(gray), gray.numel(), _dptr(sse)))
        return sse

    def deflate_columns_into(self, src, table, slots, lens):
        """lrf_deflate_columns_i8 with every offset named by the caller: src a flat int8 CUDA tensor, table an int64 array [n, 5]
        of (src_off, rows, cols, dst_off, len_off) on the host, slots a flat uint8 and lens a flat int32 CUDA tensor.  The
        library checks every range before it launches (ValueError).  Asynchronous on torch's current stream."""
        import torch
        for t, dt in ((src, torch.int8), (slots, torch.uint8), (lens, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise TypeError("deflate_columns takes an int8 source, uint8 slots and int32 lengths")
            if t.dim() != 1 or not t.is_contiguous() or not (t.is_cuda and t.device.index == self.device):
                raise ValueError(f"deflate_columns needs flat contiguous tensors on cuda:{self.device}")
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 5)
        self.use_torch_stream()
        check(self._lib.lrf_deflate_columns_i8(self._h, _dptr(src), src.numel(), table.shape[0], c_void_p(table.ctypes.data), _dptr(slots),
                                               slots.numel(), _dptr(lens), lens.numel()))

    def deflate_columns(self, src, mats):
        """The zlib stream of every column of int8 matrices, written on the device (lrf_deflate_columns_i8).  src: a flat int8
        CUDA tensor; mats: [(src_off, rows, cols)], matrix i row-major [rows, cols] at src[src_off:] -> (slots, lens): a flat
        uint8 and a flat int32 CUDA tensor laid out as deflate_table(mats) says (column j of matrix i: lens[len_off_i + j]
        bytes at slots[dst_off_i + j * deflate_bound(rows_i):]).  Asynchronous on torch's current stream."""
        import torch
        table, nbytes, ncols = deflate_table(mats)
        slots = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
        lens = torch.empty((ncols,), dtype=torch.int32, device=src.device)
        self.deflate_columns_into(src, table, slots, lens)
        return slots, lens

    def deflate_sizes_into(self, src, table, lens):
        """lrf_deflate_sizes_i8 with every offset named by the caller: src a flat int8 CUDA tensor, table an int64 array [n, 5] of
        (src_off, rows, cols, dst_off, len_off) on the host (deflate_table's layout; dst_off is not used), lens a flat int32
        CUDA tensor.  lens[len_off + j] becomes what deflate_columns_into writes there; nothing else is written.  The library
        checks every range before it launches (ValueError).  Asynchronous on torch's current stream."""
        import torch
        for t, dt in ((src, torch.int8), (lens, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise TypeError("deflate_sizes takes an int8 source and int32 lengths")
        for t in (src, lens):
            if t.dim() != 1 or not t.is_contiguous() or not (t.is_cuda and t.device.index == self.device):
                raise ValueError(f"deflate_sizes needs flat contiguous tensors on cuda:{self.device}")
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 5)
        self.use_torch_stream()
        check(self._lib.lrf_deflate_sizes_i8(self._h, _dptr(src), src.numel(), table.shape[0], c_void_p(table.ctypes.data), _dptr(lens), lens.numel()))

    def deflate_sizes(self, src, mats):
        """The length of every column's zlib stream without the stream (lrf_deflate_sizes_i8).  src, mats: as deflate_columns
        takes them -> lens, a flat int32 CUDA tensor equal to the one deflate_columns returns.  Asynchronous on torch's current
        stream."""
        import torch
        table, _, ncols = deflate_table(mats)
        lens = torch.empty((ncols,), dtype=torch.int32, device=src.device)
        self.deflate_sizes_into(src, table, lens)
        return lens

    def inflate_columns_into(self, src, table, col_off, col_len, dst, status):
        """lrf_inflate_columns_i8 with every offset named by the caller: src a flat uint8 CUDA tensor holding the zlib streams,
        table an int64 array [n, 4] of (dst_off, rows, cols, first) on the host, col_off (int64) and col_len (int32) host arrays
        with one entry per stream, dst a flat int8 and status a flat int32 CUDA tensor with one entry per stream (0, or the
        LRFI_E_* of include/lrf_hip.h).  The library checks every range before it launches (ValueError).  Asynchronous on
        torch's current stream."""
        import torch
        for t, dt in ((src, torch.uint8), (dst, torch.int8), (status, torch.int32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt:
                raise TypeError("inflate_columns takes a uint8 source, an int8 destination and int32 statuses")
            if t.dim() != 1 or not t.is_contiguous() or not (t.is_cuda and t.device.index == self.device):
                raise ValueError(f"inflate_columns needs flat contiguous tensors on cuda:{self.device}")
        table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 4)
        col_off = np.ascontiguousarray(col_off, dtype=np.int64).reshape(-1)
        col_len = np.ascontiguousarray(col_len, dtype=np.int32).reshape(-1)
        if col_off.shape != col_len.shape or status.numel() != col_off.shape[0]:
            raise ValueError(f"inflate_columns: {col_off.shape[0]} offsets, {col_len.shape[0]} lengths and {status.numel()} statuses")
        self.use_torch_stream()
        check(self._lib.lrf_inflate_columns_i8(self._h, _dptr(src), src.numel(), table.shape[0], c_void_p(table.ctypes.data),
                                               c_void_p(col_off.ctypes.data), c_void_p(col_len.ctypes.data), col_off.shape[0], _dptr(dst),
                                               dst.numel(), _dptr(status)))

    def image_metrics(self, a, b, want_ssim=True):
        """uint8 CUDA tensors a, b [B,C,H,W] -> (sse int64 [B], ssim float64 [B] or None) on the device (lrf_image_metrics_u8):
        the exact sum of squared differences and the SSIM `lrf_amd.metrics.ssim(a[i], b[i])` defines, per image"""
        import torch
        check_metrics_args(a, b, want_ssim)
        if not (a.is_cuda and b.is_cuda and a.device == b.device and a.device.index == self.device):
            raise ValueError(f"image_metrics needs both tensors on cuda:{self.device}, got {a.device} and {b.device}")
        if not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("image_metrics needs contiguous tensors")
        B, C, H, W = a.shape
        sse = torch.empty((B,), dtype=torch.int64, device=a.device)
        ssim = torch.empty((B,), dtype=torch.float64, device=a.device) if want_ssim else None
        self.use_torch_stream()
        check(self._lib.lrf_image_metrics_u8(self._h, _dptr(a), _dptr(b), B, C, H, W, _dptr(sse), _dptr(ssim)))
        return sse, ssim

    def sweep_sse(self, rgb, factors, triples):
        """The squared error of a sweep straight from its factors (lrf_qmf_sweep_sse_rgb_u8): rgb uint8 CUDA [B,3,H,W], `factors`
        one (U, V) pair per rank triple of `triples`, as encode_sweep_rgb returns them (one pair: encode_rgb's) -> int64 CUDA
        tensor [Q, B], sse[q][b] = what image_metrics(rgb, decode_rgb(U_q, V_q, H, W, triples[q]), want_ssim=False)[0][b] gives,
        without the decoded images.  Pairs that are not already consecutive views of two flat buffers are copied into such."""
        import torch
        check_sweep_sse_args(rgb, factors, triples)
        if not (rgb.is_cuda and rgb.device.index == self.device and factors[0][0].device == rgb.device):
            raise ValueError(f"sweep_sse needs its tensors on cuda:{self.device}, got {rgb.device} and {factors[0][0].device}")
        if not rgb.is_contiguous():
            raise ValueError("sweep_sse needs a contiguous image tensor")
        B, _, H, W = rgb.shape
        U, V = flat_views([f[0] for f in factors]), flat_views([f[1] for f in factors])
        sse = torch.empty((len(triples), B), dtype=torch.int64, device=rgb.device)
        R = (c_int * (3 * len(triples)))(*[int(r) for t in triples for r in t])
        self.use_torch_stream()
        check(self._lib.lrf_qmf_sweep_sse_rgb_u8(self._h, _dptr(rgb), _dptr(U), _dptr(V), B, H, W, len(triples), R, _dptr(sse)))
        return sse

    def planes_any(self, rgb, patch_size, ch, chroma=None):
        """rgb uint8 [B,3,H,W] (CUDA) -> X fp32 [B, M, N] of plane ch for patches (p, q) (None: the plane itself)"""
        import torch
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        hc, wc = (0, 0) if chroma is None else (int(chroma[0]), int(chroma[1]))
        d = plane_dims_any(H, W, patch_size, chroma)[ch]
        X = torch.empty((B, d[4], d[5]), dtype=torch.float32, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_planes_any_hw_u8(self._h, _dptr(rgb.contiguous()), B, H, W, hc, wc, p, q, ch, _dptr(X)))
        return X

    def decode_any(self, Us, Vs, H, W, patch_size, chroma=None):
        """three (U [B,M_c,R_c], V [B,N_c,R_c]) int8 CUDA pairs -> uint8 [B,3,H,W]"""
        import torch
        Us = [u.contiguous() for u in Us]
        Vs = [v.contiguous() for v in Vs]
        B = Us[0].shape[0]
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        hc, wc = (0, 0) if chroma is None else (int(chroma[0]), int(chroma[1]))
        dims = plane_dims_any(H, W, patch_size, chroma)
        for c in range(3):
            assert Us[c].shape[1] == dims[c][4] and Vs[c].shape[1] == dims[c][5] and Us[c].shape[2] == Vs[c].shape[2], \
                "factor shapes do not match the image geometry"
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=Us[0].device)
        R = (c_int * 3)(*[int(u.shape[2]) for u in Us])
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_any_hw_u8(self._h, _dptr(Us[0]), _dptr(Vs[0]), _dptr(Us[1]), _dptr(Vs[1]), _dptr(Us[2]),
                                                 _dptr(Vs[2]), B, H, W, hc, wc, p, q, R, _dptr(rgb)))
        return rgb


def _svd_methods():
    def svd_encode_rgb(self, rgb, R, sign=None):
        """rgb uint8 [B,3,H,W] (CUDA) -> (U uint8 [B,M,R], V uint8 [B,192,R], qparams float [B,4])"""
        import torch
        rgb = rgb.contiguous()
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        M = ((H + 7) // 8) * ((W + 7) // 8)
        U = torch.empty((B, M, R), dtype=torch.uint8, device=rgb.device)
        V = torch.empty((B, 192, R), dtype=torch.uint8, device=rgb.device)
        qp = torch.empty((B, 4), dtype=torch.float32, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_svd_encode_rgb_u8(self._h, _dptr(rgb), B, H, W, int(R), _dptr(sign), _dptr(U), _dptr(V), _dptr(qp)))
        return U, V, qp

    def svd_decode_rgb(self, U, V, qparams6, H, W):
        import torch
        U, V, qparams6 = U.contiguous(), V.contiguous(), qparams6.float().contiguous()
        B, _, R = U.shape
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_svd_decode_rgb_u8(self._h, _dptr(U), _dptr(V), B, H, W, int(R), _dptr(qparams6), _dptr(rgb)))
        return rgb

    def qmf_rgbspace_encode(self, rgb, R, num_iters=10, bounds=(-16, 15), sign=None, init=None):
        """qmf_encode's RGB colour-space branch: rgb uint8 [B,3,H,W] (CUDA) -> (U int8 [B,M,R], V int8 [B,192,R]).
        init = (U0 [B,M,R], V0 [B,192,R]) fp32 overrides the SVD initialisation."""
        import torch
        rgb = rgb.contiguous()
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        M = ((H + 7) // 8) * ((W + 7) // 8)
        U = torch.empty((B, M, R), dtype=torch.int8, device=rgb.device)
        V = torch.empty((B, 192, R), dtype=torch.int8, device=rgb.device)
        u0 = v0 = None
        if init is not None:
            u0, v0 = (t.to(device=rgb.device, dtype=torch.float32).contiguous() for t in init)
            assert tuple(u0.shape) == (B, M, R) and tuple(v0.shape) == (B, 192, R)
        if sign is not None:
            sign = sign.to(device=rgb.device, dtype=torch.int8).contiguous()
        self.use_torch_stream()
        check(self._lib.lrf_qmf_rgbspace_encode_u8(self._h, _dptr(rgb), B, H, W, int(R), int(num_iters), int(bounds[0]), int(bounds[1]),
                                                  _dptr(sign), _dptr(u0), _dptr(v0), _dptr(U), _dptr(V)))
        return U, V

    def qmf_rgbspace_decode(self, U, V, H, W):
        import torch
        U, V = U.contiguous(), V.contiguous()
        B, _, R = U.shape
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_rgbspace_decode_u8(self._h, _dptr(U), _dptr(V), B, H, W, int(R), _dptr(rgb)))
        return rgb

    def rgbspace_matrix_any(self, rgb, patch_size):
        """rgb uint8 [B,3,H,W] (CUDA) -> X fp32: [B, M, 3 p q] for patches (p, q), [B, 3, H, W] for patch_size None"""
        import torch
        rgb = rgb.contiguous()
        B, C, H, W = rgb.shape
        assert C == 3 and rgb.dtype == torch.uint8
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        _, _, M, N = rgbspace_dims_any(H, W, patch_size)
        X = torch.empty((B, 3, H, W) if patch_size is None else (B, M, N), dtype=torch.float32, device=rgb.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_rgbspace_matrix_u8(self._h, _dptr(rgb), B, H, W, p, q, _dptr(X)))
        return X

    def qmf_rgbspace_decode_any(self, U, V, H, W, patch_size):
        """int8 U [B,M,R] / V [B,3pq,R] (patches) or U [B,3,H,R] / V [B,3,W,R] (patch_size None) -> uint8 [B,3,H,W]"""
        import torch
        U, V = U.contiguous(), V.contiguous()
        B, R = U.shape[0], U.shape[-1]
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        _, _, M, N = rgbspace_dims_any(H, W, patch_size)
        want_u, want_v = ((B, 3, H, R), (B, 3, W, R)) if patch_size is None else ((B, M, R), (B, N, R))
        if tuple(U.shape) != want_u or tuple(V.shape) != want_v or U.dtype != torch.int8 or V.dtype != torch.int8:
            raise ValueError(f"factor shapes {tuple(U.shape)} / {tuple(V.shape)} do not match the geometry {want_u} / {want_v}")
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_rgbspace_decode_any_u8(self._h, _dptr(U), _dptr(V), B, H, W, p, q, int(R), _dptr(rgb)))
        return rgb

    def quantize_u8(self, T):
        """quantize(t, uint8) of each T[b] as a whole (utils.py:185-220): fp32 CUDA [B, ...] -> (uint8 same shape, qparams [B,2])"""
        import torch
        T = T.float().contiguous()
        B = T.shape[0]
        per = T[0].numel()
        Q = torch.empty(T.shape, dtype=torch.uint8, device=T.device)
        qp = torch.empty((B, 2), dtype=torch.float32, device=T.device)
        self.use_torch_stream()
        check(self._lib.lrf_quantize_u8(self._h, _dptr(T), B, per, _dptr(Q), _dptr(qp)))
        return Q, qp

    def svd_decode_any(self, U, V, H, W, patch_size, qparams6=None):
        """uint8 factors + qparams6 [B,6], or float32 factors (qparams6 None) -> uint8 [B,3,H,W]; layouts as qmf_rgbspace_decode_any"""
        import torch
        U, V = U.contiguous(), V.contiguous()
        B, R = U.shape[0], U.shape[-1]
        is_float = U.dtype == torch.float32
        assert U.dtype == V.dtype and (is_float or U.dtype == torch.uint8)
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        _, _, M, N = rgbspace_dims_any(H, W, patch_size)
        want_u, want_v = ((B, 3, H, R), (B, 3, W, R)) if patch_size is None else ((B, M, R), (B, N, R))
        if tuple(U.shape) != want_u or tuple(V.shape) != want_v:
            raise ValueError(f"factor shapes {tuple(U.shape)} / {tuple(V.shape)} do not match the geometry {want_u} / {want_v}")
        if not is_float:
            qparams6 = qparams6.float().contiguous()
            assert tuple(qparams6.shape) == (B, 6)
        rgb = torch.empty((B, 3, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_svd_decode_any_u8(self._h, _dptr(U), _dptr(V), int(is_float), B, H, W, p, q, int(R),
                                              None if is_float else _dptr(qparams6), _dptr(rgb)))
        return rgb

    def encode_gray(self, gray, R, num_iters=10, bounds=(-16, 15), sign=None, init=None):
        """lrf_qmf_encode_gray_u8: gray uint8 [B,H,W] (CUDA) -> (U int8 [B,M,R], V int8 [B,64,R]); sign int8 [B,R];
        init = (U0 [B,M,R], V0 [B,64,R]) fp32 overrides the SVD initialisation"""
        import torch
        gray = gray.contiguous()
        B, H, W = gray.shape
        assert gray.dtype == torch.uint8
        _, _, M, N = chan_dims(H, W, 1, (8, 8))
        U = torch.empty((B, M, R), dtype=torch.int8, device=gray.device)
        V = torch.empty((B, N, R), dtype=torch.int8, device=gray.device)
        u0 = v0 = None
        if init is not None:
            u0, v0 = (t.to(device=gray.device, dtype=torch.float32).contiguous() for t in init)
            assert tuple(u0.shape) == (B, M, R) and tuple(v0.shape) == (B, N, R)
        if sign is not None:
            sign = sign.to(device=gray.device, dtype=torch.int8).contiguous()
            assert tuple(sign.shape) == (B, R)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_encode_gray_u8(self._h, c_void_p(gray.data_ptr()), B, H, W, int(R), int(num_iters), int(bounds[0]), int(bounds[1]),
                                              _dptr(sign), _dptr(u0), _dptr(v0), _dptr(U), _dptr(V)))
        return U, V

    def decode_gray(self, U, V, H, W):
        """lrf_qmf_decode_gray_u8: int8 U [B,M,R], V [B,64,R] -> uint8 [B,H,W]"""
        import torch
        U, V = U.contiguous(), V.contiguous()
        B, R = U.shape[0], U.shape[-1]
        _, _, M, N = chan_dims(H, W, 1, (8, 8))
        if tuple(U.shape) != (B, M, R) or tuple(V.shape) != (B, N, R) or U.dtype != torch.int8 or V.dtype != torch.int8:
            raise ValueError(f"factor shapes {tuple(U.shape)} / {tuple(V.shape)} do not match the geometry {(B, M, R)} / {(B, N, R)}")
        gray = torch.empty((B, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_decode_gray_u8(self._h, _dptr(U), _dptr(V), B, H, W, int(R), _dptr(gray)))
        return gray

    def chan_matrix(self, img, patch_size):
        """img uint8 [B,C,H,W] (CUDA) -> X fp32: [B, M, C p q] for patches (p, q), [B, C, H, W] for patch_size None"""
        import torch
        img = img.contiguous()
        B, C, H, W = img.shape
        assert img.dtype == torch.uint8
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        _, _, M, N = chan_dims(H, W, C, patch_size)
        X = torch.empty((B, C, H, W) if patch_size is None else (B, M, N), dtype=torch.float32, device=img.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_chan_matrix_u8(self._h, c_void_p(img.data_ptr()), B, C, H, W, p, q, _dptr(X)))
        return X

    def chan_decode(self, U, V, C, H, W, patch_size):
        """int8 U [B,M,R] / V [B,C p q,R] (patches) or U [B,C,H,R] / V [B,C,W,R] (patch_size None) -> uint8 [B,C,H,W]"""
        import torch
        U, V = U.contiguous(), V.contiguous()
        B, R = U.shape[0], U.shape[-1]
        p, q = (0, 0) if patch_size is None else (int(patch_size[0]), int(patch_size[1]))
        _, _, M, N = chan_dims(H, W, C, patch_size)
        want_u, want_v = ((B, C, H, R), (B, C, W, R)) if patch_size is None else ((B, M, R), (B, N, R))
        if tuple(U.shape) != want_u or tuple(V.shape) != want_v or U.dtype != torch.int8 or V.dtype != torch.int8:
            raise ValueError(f"factor shapes {tuple(U.shape)} / {tuple(V.shape)} do not match the geometry {want_u} / {want_v}")
        out = torch.empty((B, C, H, W), dtype=torch.uint8, device=U.device)
        self.use_torch_stream()
        check(self._lib.lrf_qmf_chan_decode_u8(self._h, _dptr(U), _dptr(V), B, C, H, W, p, q, int(R), _dptr(out)))
        return out

    Context.encode_gray = encode_gray
    Context.decode_gray = decode_gray
    Context.chan_matrix = chan_matrix
    Context.chan_decode = chan_decode
    Context.quantize_u8 = quantize_u8
    Context.svd_decode_any = svd_decode_any
    Context.rgbspace_matrix_any = rgbspace_matrix_any
    Context.qmf_rgbspace_decode_any = qmf_rgbspace_decode_any
    Context.svd_encode_rgb = svd_encode_rgb
    Context.svd_decode_rgb = svd_decode_rgb
    Context.qmf_rgbspace_encode = qmf_rgbspace_encode
    Context.qmf_rgbspace_decode = qmf_rgbspace_decode


_svd_methods()


class _BorrowedContext(Context):
    """A Context view of an lrf_ctx owned by something else (a pipe's slot): profiling calls only, never destroyed here."""

    def __init__(self, handle, device):
        self._lib = load()
        self._h = c_void_p(handle)
        self.device = int(device)

    def close(self):
        self._h = c_void_p()


def _hptr(t):
    """host pointer of a contiguous torch CPU tensor / numpy array, or None"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"], "expected a C-contiguous array"
        return c_void_p(t.ctypes.data)
    assert (not t.is_cuda) and t.is_contiguous(), "expected a contiguous CPU tensor"
    return c_void_p(t.data_ptr())


class Pipe:
    """lrf_pipe: the host -> host pipelined encoder (include/lrf_hip.h).  Host tensors in, int8 factors back on the
    host; sub-batches stream through `slots` independent encoder contexts so that uploads, kernels and downloads
    overlap.  Not thread-safe; one per (host thread, device)."""

    def __init__(self, device=0, slots=2, sub_batch=0):
        import torch
        if not torch.cuda.is_available():
            raise LrfError("lrf_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self._lib = load()
        self._h = c_void_p()
        self.device = int(device)
        check(self._lib.lrf_pipe_create(self.device, int(slots), int(sub_batch), ctypes.byref(self._h)))
        self.slots = int(self._lib.lrf_pipe_slots(self._h))

    def close(self):
        if self._h:
            self._lib.lrf_pipe_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slot_context(self, slot):
        return _BorrowedContext(self._lib.lrf_pipe_slot_ctx(self._h, int(slot)), self.device)

    def workspace_bytes(self):
        return int(self._lib.lrf_pipe_workspace_bytes(self._h))

    def _prepare(self, rgb, ranks, sign, out):
        import torch
        assert (not rgb.is_cuda) and rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[1] == 3, \
            "expected a uint8 CPU tensor [B,3,H,W]"
        rgb = rgb.contiguous()
        B, _, H, W = rgb.shape
        dims = plane_dims(H, W)
        nu, nv = sum(d[4] * int(r) for d, r in zip(dims, ranks)), 64 * sum(int(r) for r in ranks)
        if out is None:
            pin = rgb.is_pinned()
            U = torch.empty((B, nu), dtype=torch.int8, pin_memory=pin)
            V = torch.empty((B, nv), dtype=torch.int8, pin_memory=pin)
        else:
            U, V = out
            for t, n, name in ((U, nu, "U"), (V, nv, "V")):
                if t.is_cuda or t.dtype != torch.int8 or not t.is_contiguous() or tuple(t.shape) != (B, n):
                    raise ValueError(f"out {name} must be a contiguous int8 CPU tensor of shape {(B, n)}")
        if sign is not None:
            sign = torch.as_tensor(sign, dtype=torch.int8).reshape(-1, sum(int(r) for r in ranks))
            sign = sign.expand(B, -1).contiguous()
        R = (c_int * 3)(*[int(r) for r in ranks])
        return rgb, B, H, W, R, sign, U, V

    def encode_rgb_host(self, rgb, ranks, K, lo, hi, sign=None, out=None):
        """rgb uint8 CPU tensor [B,3,H,W] (pinned for full speed) -> (U int8 [B, sum M_c R_c], V int8 [B, 64 sum R_c])
        CPU tensors; returns when they are complete."""
        rgb, B, H, W, R, sign, U, V = self._prepare(rgb, ranks, sign, out)
        check(self._lib.lrf_pipe_qmf_encode_rgb_u8_host(self._h, _hptr(rgb), B, H, W, R, int(K), int(lo), int(hi), _hptr(sign),
                                                        _hptr(U), _hptr(V)))
        return U, V

    def encode_rgb_host_iter(self, rgb, ranks, K, lo, hi, sign=None, out=None):
        """Generator form: enqueues the whole batch, then yields (first_image, n_images, U, V) as each sub-batch lands on
        the host (U, V are the full output tensors; rows [first, first + n) are final at that point)."""
        rgb, B, H, W, R, sign, U, V = self._prepare(rgb, ranks, sign, out)
        n_sub = c_int()
        rc = self._lib.lrf_pipe_qmf_encode_submit(self._h, _hptr(rgb), B, H, W, R, int(K), int(lo), int(hi), _hptr(sign), _hptr(U),
                                                  _hptr(V), ctypes.byref(n_sub))
        try:
            check(rc)
            while True:
                first, n = c_i64(), c_i64()
                check(self._lib.lrf_pipe_wait_next(self._h, ctypes.byref(first), ctypes.byref(n)))
                if n.value == 0:
                    return
                yield int(first.value), int(n.value), U, V
        finally:  # never leave copies into the caller's buffers in flight (an abandoned generator, an error)
            n = c_i64(1)
            for _ in range(max(1, int(n_sub.value)) + 1):  # (a piece that reports a failed launch still counts as waited for)
                self._lib.lrf_pipe_wait_next(self._h, None, ctypes.byref(n))
                if not n.value:
                    break


_contexts = {}
_pipes = {}


def pipe(device=None, slots=2, sub_batch=0) -> Pipe:
    """The cached pipe of the calling THREAD for (device, slots, sub_batch).  A Pipe is a per-(host thread, device) object
    (its slot buffers, submission cursor and sign table are not locked, and ctypes releases the GIL inside its calls), so
    two Python threads encoding at once each get a pipe of their own."""
    import threading

    import torch
    if not torch.cuda.is_available():
        raise LrfError("lrf_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    if device is None:
        device = torch.cuda.current_device()
    device = torch.device("cuda", device).index if not isinstance(device, int) else device
    key = (threading.get_ident(), device, int(slots), int(sub_batch))
    with _lock:
        p = _pipes.get(key)
    if p is None:
        p = Pipe(device, slots, sub_batch)
        with _lock:
            _pipes[key] = p
    return p


def context(device=None) -> Context:
    """The cached per-device context of the calling process."""
    import torch
    if not torch.cuda.is_available():
        raise LrfError("lrf_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    if device is None:
        device = torch.cuda.current_device()
    device = torch.device("cuda", device).index if not isinstance(device, int) else device
    with _lock:
        ctx = _contexts.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _contexts[device] = ctx
    return ctx
