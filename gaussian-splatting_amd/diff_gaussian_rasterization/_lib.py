"""ctypes binding of libgsr_hip.so (include/gsr.h).

This file is the "reference-side binding" INTEGRATION.md describes: it replaces the pybind11 module
`diff_gaussian_rasterization._C` of the reference's un-vendored submodule (call sites
gaussian_renderer/__init__.py:14,91-110).  There is NO fallback: if the shared library is missing or was
not built for this GPU, loading raises -- the product path never routes through a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libgsr_hip.so")

GSR_OK = 0
ABI_VERSION = 4
STAGES = ["preprocess", "depth_sort", "scan", "emit", "tile_sort", "ranges", "render", "render_bwd", "preprocess_bwd",
          "gather_bwd", "color", "r_wait"]


class GsrRasterSettings(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("bg", C.c_void_p), ("scale_modifier", C.c_float),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("sh_degree", C.c_int32), ("campos", C.c_void_p),
        ("prefiltered", C.c_int32), ("debug", C.c_int32), ("antialiasing", C.c_int32),
        ("tile_y0", C.c_int32), ("tile_y1", C.c_int32), ("no_backward", C.c_int32),
        ("sh_dc", C.c_void_p), ("dL_dsh_dc", C.c_void_p),
    ]


class GsrForwardViews(C.Structure):
    _fields_ = [("splats", C.c_void_p), ("tiles_touched", C.c_void_p), ("depth_order", C.c_void_p),
                ("point_list", C.c_void_p), ("ranges", C.c_void_p), ("final_T", C.c_void_p),
                ("n_contrib", C.c_void_p), ("tile_scan", C.c_void_p)]


RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_lib: Optional[C.CDLL] = None


class GsrError(RuntimeError):
    pass


def lib_path() -> str:
    return os.environ.get("GSR_LIB", _LIB_PATH)



class ShAdam(C.Structure):
    """GsrShAdam of include/gsr.h (gsr_backward_preprocess_sh_adam)."""
    _fields_ = [("dc_exp_avg", C.c_void_p), ("dc_exp_avg_sq", C.c_void_p), ("rest_exp_avg", C.c_void_p), ("rest_exp_avg_sq", C.c_void_p),
                ("lr_dc", C.c_double), ("lr_rest", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("step_dc", C.c_int32), ("step_rest", C.c_int32), ("sparse", C.c_int32), ("reserved", C.c_int32)]


class CameraGrads(C.Structure):
    """GsrCameraGrads of include/gsr.h (gsr_backward_preprocess_camera)."""
    _fields_ = [("dL_dviewmatrix", C.c_void_p), ("dL_dprojmatrix", C.c_void_p), ("dL_dcampos", C.c_void_p), ("scratch", C.c_void_p)]


class CompositeOut(C.Structure):
    """GsrCompositeOut of include/gsr.h (gsr_rasterize_forward_composite)."""
    _fields_ = [("out_alpha", C.c_void_p), ("bg_image", C.c_void_p)]


class CompositeGrads(C.Structure):
    """GsrCompositeGrads of include/gsr.h (gsr_backward_blend_composite)."""
    _fields_ = [("dL_dout_alpha", C.c_void_p), ("bg_image", C.c_void_p), ("dL_dbg_image", C.c_void_p), ("dL_dbg", C.c_void_p),
                ("scratch", C.c_void_p)]


class ContribOut(C.Structure):
    """GsrContribOut of include/gsr.h (gsr_contribution_stats)."""
    _fields_ = [("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("pixel_count", C.c_void_p), ("accumulate", C.c_int32),
                ("reserved", C.c_int32)]


class PixelProbeOut(C.Structure):
    """GsrPixelProbeOut of include/gsr.h (gsr_pixel_probe)."""
    _fields_ = [("expected_depth", C.c_void_p), ("median_depth", C.c_void_p), ("median_id", C.c_void_p), ("top_id", C.c_void_p),
                ("top_weight", C.c_void_p), ("count", C.c_void_p), ("threshold", C.c_float), ("reserved", C.c_int32)]


class DistortionOut(C.Structure):
    """GsrDistortionOut of include/gsr.h (gsr_distortion)."""
    _fields_ = [("distortion", C.c_void_p), ("saved", C.c_void_p), ("depth_mode", C.c_int32), ("reserved", C.c_int32)]


class AdamTensor(C.Structure):
    """GsrAdamTensor of include/gsr.h (gsr_adam_step_multi)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step", C.c_int32),
                ("reserved", C.c_int32)]

class SparseAdamTensor(C.Structure):
    """GsrSparseAdamTensor of include/gsr.h (gsr_sparse_adam_step_multi)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("M", C.c_int64),
                ("lr", C.c_double), ("eps", C.c_double)]


_vp, _i32p, _i64p, _RS = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(GsrRasterSettings)
_BUFFERS = [RESIZE_FN, _vp] * 3      # geometry, binning and image buffer: resize callback + user pointer each
_RECORDS_OUT = _BUFFERS + [_vp, _vp, _i32p, _vp]      # out_color, out_invdepth, num_rendered, stream

# name -> (restype, argtypes) of every function include/gsr.h declares, in its parameter order (tests/test_abi_cpu.py holds the arities to
# the header)
SIGNATURES = {
    "gsr_abi_version": (C.c_int, []),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_geometry_bytes": (C.c_size_t, [C.c_int]),
    "gsr_binning_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "gsr_image_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "gsr_backward_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "gsr_rasterize_forward": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 7 + _BUFFERS + [_vp, _vp, _vp, _i32p, _vp]),
    "gsr_rasterize_backward": (C.c_int, [_RS, C.c_int, C.c_int, C.c_int32] + [_vp] * 8 + [_vp] * 5 + [_vp] * 9
                               + [C.POINTER(C.c_void_p), _vp]),
    "gsr_backward_blend": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 6 + [C.POINTER(C.c_void_p), _vp]),
    "gsr_backward_preprocess": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 10 + [_vp] * 9),
    "gsr_camera_grad_scratch_bytes": (C.c_size_t, [C.c_int]),
    "gsr_backward_preprocess_camera": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 10 + [_vp] * 8 + [C.POINTER(CameraGrads), _vp]),
    "gsr_rasterize_forward_composite": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 7 + _BUFFERS + [_vp, _vp, _vp, _i32p, C.POINTER(CompositeOut), _vp]),
    "gsr_composite_grad_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "gsr_backward_blend_composite": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 6 + [C.POINTER(C.c_void_p), C.POINTER(CompositeGrads), _vp]),
    "gsr_backward_blend_abs": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 6 + [C.POINTER(C.c_void_p), C.POINTER(CompositeGrads), _vp]),
    "gsr_absgrad_from_records": (C.c_int, [_RS, C.c_int, _vp, _vp, _vp]),
    "gsr_contribution_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "gsr_contribution_stats": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 5 + [C.POINTER(ContribOut), _vp]),
    "gsr_pixel_probe": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 3 + [C.POINTER(PixelProbeOut), _vp]),
    "gsr_render_features": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 4 + [C.c_int, _vp, _vp]),
    "gsr_feature_grad_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "gsr_render_features_backward": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 4 + [C.c_int, _vp, _vp, _vp]),
    "gsr_render_features_backward_geometry": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 5 + [C.c_int, _vp, C.POINTER(C.c_void_p), _vp]),
    "gsr_distortion": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 3 + [C.POINTER(DistortionOut), _vp]),
    "gsr_distortion_backward": (C.c_int, [_RS, C.c_int, C.c_int32] + [_vp] * 5 + [C.c_int, _vp, C.POINTER(C.c_void_p), _vp]),
    "gsr_preprocess_forward": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 11),
    "gsr_rasterize_from_splats": (C.c_int, [_RS, C.c_int, _vp] + _RECORDS_OUT),
    "gsr_route_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "gsr_route_count": (C.c_int, [C.c_int, _vp, C.c_int, _i32p, _vp, _vp, _vp]),
    "gsr_route_pack": (C.c_int, [C.c_int, _vp, C.c_int, _i32p, _i64p, _vp, _vp, _vp, _vp]),
    "gsr_rasterize_from_packed": (C.c_int, [_RS, C.c_int, _vp] + _RECORDS_OUT),
    "gsr_route_return": (C.c_int, [C.c_int, C.c_int, _i64p, _vp, _vp, _vp, _vp]),
    "gsr_route_pack_fixed": (C.c_int, [C.c_int, _vp, C.c_int, _i32p, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "gsr_rasterize_from_segments": (C.c_int, [_RS, C.c_int, C.c_int, _vp] + _RECORDS_OUT),
    "gsr_backward_preprocess_sh_adam": (C.c_int, [_RS, C.c_int, C.c_int] + [_vp] * 9 + [_vp] * 6 + [C.POINTER(ShAdam), _vp]),
    "gsr_adam_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _vp]),
    "gsr_adam_step_multi": (C.c_int, [C.POINTER(AdamTensor), C.c_int32, _vp]),
    "gsr_sparse_adam_step": (C.c_int, [_vp] * 5 + [C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, _vp]),
    "gsr_sparse_adam_step_multi": (C.c_int, [C.POINTER(SparseAdamTensor), C.c_int32, _vp, C.c_int64, C.c_double, C.c_double, _vp]),
    "gsr_density_stats": (C.c_int, [C.c_int] + [_vp] * 7),
    "gsr_mcmc_inject_noise": (C.c_int, [C.c_int] + [_vp] * 5 + [C.c_int, C.c_float, C.c_float, C.c_float, _vp]),
    "gsr_mcmc_relocation": (C.c_int, [C.c_int] + [_vp] * 5 + [_vp]),
    "gsr_bilagrid_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "gsr_bilagrid_slice": (C.c_int, [C.c_int] * 5 + [_vp] * 4),
    "gsr_bilagrid_slice_backward": (C.c_int, [C.c_int] * 5 + [_vp] * 6 + [C.c_size_t, _vp]),
    "gsr_bilagrid_tv_partial_count": (C.c_int64, [C.c_int] * 4),
    "gsr_bilagrid_tv": (C.c_int, [C.c_int] * 4 + [_vp] * 4),
    "gsr_bilagrid_tv_backward": (C.c_int, [C.c_int] * 4 + [_vp] * 4),
    "gsr_gaussian_normals": (C.c_int, [C.c_int] + [_vp] * 6),
    "gsr_gaussian_normals_backward": (C.c_int, [C.c_int] + [_vp] * 7),
    "gsr_depth_normals": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float] + [_vp] * 3),
    "gsr_depth_normals_backward": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float] + [_vp] * 4),
    "gsr_normal_loss_partial_count": (C.c_int64, [C.c_int] * 2),
    "gsr_normal_loss": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float] + [_vp] * 6),
    "gsr_normal_loss_backward": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float] + [_vp] * 7),
    "gsr_mip_filter_scratch_bytes": (C.c_size_t, [C.c_int]),
    "gsr_mip_filter_3d": (C.c_int, [C.c_int, _vp, C.c_int] + [_vp] * 5),
    "gsr_mip_activations": (C.c_int, [C.c_int] + [_vp] * 6),
    "gsr_mip_activations_backward": (C.c_int, [C.c_int] + [_vp] * 8),
    "gsr_vq_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "gsr_vq_assign": (C.c_int, [C.c_int] * 3 + [_vp] * 6),
    "gsr_vq_update": (C.c_int, [C.c_int] * 3 + [_vp] * 7),
    "gsr_tsdf_integrate": (C.c_int, [C.c_int] * 3 + [C.c_float] * 6 + [C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 6),
    "gsr_mesh_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "gsr_mesh_count": (C.c_int, [C.c_int] * 3 + [_vp, _vp, C.c_float, _vp, _vp, _vp]),
    "gsr_mesh_emit": (C.c_int, [C.c_int] * 3 + [C.c_float] * 4 + [_vp] * 3 + [C.c_int] * 2 + [_vp] * 4),
    "gsr_meshops_scratch_bytes": (C.c_size_t, [C.c_int] * 2),
    "gsr_mesh_components": (C.c_int, [C.c_int] * 2 + [_vp] * 5),
    "gsr_mesh_components_rounds": (C.c_int, []),
    "gsr_mesh_compact_count": (C.c_int, [C.c_int] * 2 + [_vp] * 5),
    "gsr_mesh_compact_emit": (C.c_int, [C.c_int] * 2 + [_vp] * 5 + [C.c_int] * 2 + [_vp] * 4),
    "gsr_mesh_vertex_normals": (C.c_int, [C.c_int] * 2 + [_vp] * 5),
    "gsr_mesh_smooth": (C.c_int, [C.c_int] * 2 + [_vp, _vp, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp]),
    "gsr_knn_scratch_bytes": (C.c_size_t, [C.c_int]),
    "gsr_knn_mean_dist2": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp]),
    "gsr_ssim_forward": (C.c_int, [C.c_int] * 3 + [_vp] * 7),
    "gsr_ssim_backward": (C.c_int, [C.c_int] * 3 + [_vp] * 8),
    "gsr_ssim_partial_count": (C.c_int64, [C.c_int] * 3),
    "gsr_ssim_mean_forward": (C.c_int, [C.c_int] * 3 + [_vp] * 8),
    "gsr_ssim_mean_backward": (C.c_int, [C.c_int] * 3 + [_vp] * 8),
    "gsr_train_loss_forward": (C.c_int, [C.c_int] * 3 + [_vp, _vp, C.c_float] + [_vp] * 6),
    "gsr_train_loss_backward": (C.c_int, [C.c_int] * 3 + [_vp, _vp, _vp, C.c_float] + [_vp] * 5),
    "gsr_mark_visible": (C.c_int, [C.c_int] + [_vp] * 5),
    "gsr_forward_views": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(GsrForwardViews)]),
    "gsr_profile_enable": (C.c_int, [C.c_int]),
    "gsr_profile_reset": (C.c_int, []),
    "gsr_profile_read": (C.c_int, [C.POINTER(C.c_float), _i32p, C.c_int]),
    "gsr_profile_counters": (C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_int]),
    "gsr_profile_trace": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "gsr_set_option": (C.c_int, [C.c_char_p, C.c_int]),
}
EXPORTS = list(SIGNATURES)


def load() -> C.CDLL:
    """Load libgsr_hip.so.  torch must own the HIP runtime: torch bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7) and our library NEEDs the same SONAME, so importing torch first makes both resolve to
    one runtime -- stream handles and device pointers are then interchangeable."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise GsrError(f"{path} not found: build it with `python gaussian-splatting_amd/build.py` "
                       f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first)
    except Exception:  # pragma: no cover - torch-less use (pure C hosts) links /opt/rocm's runtime
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    lib.gsr_abi_version.restype = C.c_int
    # the version is checked BEFORE any other symbol is bound: an older library (tools/build_prev_lib.sh, GSR_LIB=...) fails
    # with this message instead of an AttributeError on a symbol it does not have yet
    mismatch_ok = os.environ.get("GSR_ALLOW_ABI_MISMATCH") == "1"
    if lib.gsr_abi_version() != ABI_VERSION and not mismatch_ok:
        raise GsrError(f"{path}: ABI version {lib.gsr_abi_version()} != {ABI_VERSION} (set GSR_ALLOW_ABI_MISMATCH=1 to bind the "
                       f"symbols both versions share, for A/B runs of an older revision)")
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    if missing and not mismatch_ok:
        raise GsrError(f"{path} does not export {missing}")
    for name, (restype, argtypes) in SIGNATURES.items():
        if name not in missing:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    # measurement hook: GSR_OPTIONS="name=value,name=value" applies gsr_set_option switches at load time (A/B runs of the
    # test-suite and of bench.py without editing them); unknown names raise
    for kv in filter(None, os.environ.get("GSR_OPTIONS", "").split(",")):
        k, v = kv.split("=")
        check(lib.gsr_set_option(k.strip().encode(), int(v)), f"GSR_OPTIONS {kv}")
    return lib

def check(rc: int, what: str) -> None:
    if rc != GSR_OK:
        msg = load().gsr_last_error()
        raise GsrError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def set_option(name: str, value: int) -> None:
    check(load().gsr_set_option(name.encode(), int(value)), "gsr_set_option")


def profile_enable(on, counters: bool = False, trace: bool = False) -> None:
    """on: per-stage HIP events; counters: the blend kernels' work counters (they slow the kernels: use a separate pass);
    trace: per-wave start / end / placement records of the blend kernels instead of the counters (profile_trace)."""
    load().gsr_profile_enable((1 if on else 0) | (2 if counters else 0) | (4 if trace else 0))


def profile_trace(max_waves: int = 65536):
    """[n, 4] uint64: start, end (100 MHz ticks), placement (HW_ID | XCC << 32 | kernel << 40), steps of the most recent blend launches' waves."""
    import numpy as np
    buf = np.zeros((max_waves, 4), dtype=np.uint64)
    n = load().gsr_profile_trace(buf.ctypes.data_as(C.POINTER(C.c_uint64)), int(max_waves))
    if n < 0:
        raise GsrError("gsr_profile_trace failed")
    return buf[:n]


def profile_reset() -> None:
    load().gsr_profile_reset()


def profile_counters(reset: bool = True) -> dict:
    out = (C.c_uint64 * 6)()
    check(load().gsr_profile_counters(out, 6, 1 if reset else 0), "gsr_profile_counters")
    return {"fwd_steps": int(out[0]), "fwd_batches": int(out[1]), "bwd_steps": int(out[2]), "bwd_batches": int(out[3]),
            "fwd_max_wave_steps": int(out[4]), "bwd_max_wave_steps": int(out[5])}


def profile_read() -> dict:
    n = len(STAGES)
    ms = (C.c_float * n)()
    cnt = (C.c_int32 * n)()
    load().gsr_profile_read(ms, cnt, n)
    return {STAGES[i]: {"ms": float(ms[i]), "launches": int(cnt[i])} for i in range(n)}
